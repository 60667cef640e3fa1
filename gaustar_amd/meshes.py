"""Surface-mesh side of a refinement iteration (gaustar_trainers/refine.py:676-706) without pytorch3d.

GauSTAR's trainer reads four things of pytorch3d on its mesh: `Meshes(verts=[v], faces=[f])` with `verts_packed`,
`edges_packed` and `faces_areas_packed`, `pytorch3d.loss.mesh_normal_consistency` and
`pytorch3d.loss.mesh_laplacian_smoothing`.  This module restates them for ONE mesh, so that refine.py:681-706 runs unchanged
after swapping two imports:

    from gaustar_amd.meshes import Meshes, mesh_laplacian_smoothing, mesh_normal_consistency

`MeshTopology` holds what depends only on the faces -- pytorch3d's edge order, the face pairs of every edge and a
vertex-major incidence list -- built once per face tensor with torch operations on its device; the per-iteration work
(values and gradients of the three terms) is the fused HIP op gaustar_amd.losses.surface_mesh_loss.

Deliberately NOT a package named `pytorch3d`: that would shadow a real install.
"""
from __future__ import annotations

from functools import cached_property

import torch

_TOPO_ATTR = "_gsr_mesh_topology"   # set on the faces tensor OBJECT: (version, n_verts, MeshTopology)


def _csr(owner: torch.Tensor, item: torch.Tensor, n_owners: int, n_items: int) -> tuple:
    """(offsets [n_owners + 1], items) int32: every owner's items (int64 in [0, n_items)) in ascending order, owner-major."""
    key, _ = torch.sort(owner * max(n_items, 1) + item)
    counts = torch.bincount(owner, minlength=n_owners)
    off = torch.cat([torch.zeros(1, dtype=torch.long, device=owner.device), torch.cumsum(counts, 0)])
    return off.int().contiguous(), (key % max(n_items, 1)).int().contiguous()


class MeshTopology:
    """The fixed part of a single triangle mesh (faces [F,3] int64 in [0, n_verts)):

      edges_packed [E,2] int64 (and `edges` int32): pytorch3d's Meshes.edges_packed() -- the face-edges (v1,v2) of every
          face, then (v2,v0), then (v0,v1), each sorted to (min, max), deduplicated by torch.unique on V*min + max;
      face_to_edge [F,3] int64: Meshes.faces_packed_to_edges_packed(), [f, k] = the edge opposite corner k;
      pairs [Q,4] int32: (e0, e1, a, b) for every pair of faces sharing an edge (e0, e1) -- n(n-1)/2 pairs for an edge of
          n faces, in the order of torch.combinations over the edge's face-edges sorted by edge -- with a, b the corners of
          the two faces not on the edge; pair_edge [Q] int64 the pair's edge;
      csr_offsets [V+1], csr_entries int32: every (vertex, element, role) incidence, vertex-major, entry = element * 4 +
          role over the element index space pairs [0, Q), edges [Q, Q + E), faces [Q + E, Q + E + F) (include/gsr.h);
      vertex_neighbours, vertex_face_csr: two more vertex-major lists, built on first use.

    Built with torch operations on the faces' device (host synchronisations: this is not the hot path).  Use
    MeshTopology.of(faces, n_verts) for the cached instance."""

    def __init__(self, faces: torch.Tensor, n_verts: int):
        if faces.dim() != 2 or faces.size(1) != 3:
            raise RuntimeError(f"faces must have dimensions (F, 3), got {tuple(faces.shape)}")
        V = int(n_verts)
        f = faces.detach().long().contiguous()
        F = int(f.size(0))
        dev = f.device
        if F and (int(f.min()) < 0 or int(f.max()) >= V):
            raise IndexError(f"faces hold vertex indices outside [0, {V})")
        self.V, self.F = V, F
        self.faces = f.int().contiguous()
        v0, v1, v2 = f[:, 0], f[:, 1], f[:, 2]
        e = torch.cat([torch.stack([v1, v2], 1), torch.stack([v2, v0], 1), torch.stack([v0, v1], 1)], 0)
        e, _ = e.sort(dim=1)
        u, inverse = torch.unique(V * e[:, 0] + e[:, 1], return_inverse=True)
        self.edges_packed = torch.stack([u // V, u % V], 1) if F else torch.zeros(0, 2, dtype=torch.long, device=dev)
        self.edges = self.edges_packed.int().contiguous()
        self.E = E = int(self.edges_packed.size(0))
        self.face_to_edge = inverse.view(3, F).t().contiguous() if F else torch.zeros(0, 3, dtype=torch.long, device=dev)

        # face pairs of every edge: the 3F face-edges in face_to_edge.reshape(F*3) order, sorted by edge
        eid, order = torch.sort(self.face_to_edge.reshape(-1), stable=True)
        opp = f.reshape(-1)[order]                                   # the corner opposite face-edge (f, k) is faces[f, k]
        cnt = torch.bincount(eid, minlength=E)
        start = torch.cumsum(cnt, 0) - cnt
        pos = torch.arange(eid.numel(), device=dev) - start[eid]     # index of the face-edge within its edge
        n_after = cnt[eid] - 1 - pos                                 # partners later in the same edge
        first = torch.repeat_interleave(torch.arange(eid.numel(), device=dev), n_after)
        self.Q = Q = int(first.numel())
        run0 = torch.cumsum(n_after, 0) - n_after
        second = first + 1 + (torch.arange(Q, device=dev) - torch.repeat_interleave(run0, n_after))
        self.pair_edge = eid[first]
        self.pairs = torch.stack([self.edges_packed[self.pair_edge, 0], self.edges_packed[self.pair_edge, 1], opp[first],
                                  opp[second]], 1).int().contiguous()

        # vertex-major incidence list: entries sorted by (vertex, element * 4 + role)
        T4 = 4 * (Q + E + F)
        if T4 >= 2 ** 31:
            raise RuntimeError("mesh too large for the int32 incidence list")
        ar = lambda n: torch.arange(n, device=dev, dtype=torch.long)
        role = lambda n: ar(n)[None, :]
        vid = torch.cat([self.pairs.long().reshape(-1), self.edges_packed.reshape(-1), f.reshape(-1)])
        code = torch.cat([ar(4 * Q), ((Q + ar(E))[:, None] * 4 + role(2)).reshape(-1), ((Q + E + ar(F))[:, None] * 4 + role(3)).reshape(-1)])
        self.csr_offsets, self.csr_entries = _csr(vid, code, V, T4)

    @cached_property
    def vertex_neighbours(self) -> tuple:
        """(offsets [V+1], neighbours) int32: trimesh's vertex_neighbors from the edges, each list in ascending order."""
        e = self.edges_packed
        return _csr(torch.cat([e[:, 0], e[:, 1]]), torch.cat([e[:, 1], e[:, 0]]), self.V, self.V)

    @cached_property
    def vertex_face_csr(self) -> tuple:
        """(offsets [V+1], entries [3F]) int32: every vertex's incidences face * 3 + corner in ascending face order."""
        return _csr(self.faces.reshape(-1).long(), torch.arange(3 * self.F, device=self.device), self.V, 3 * self.F)

    @property
    def device(self):
        return self.faces.device

    @classmethod
    def of(cls, faces: torch.Tensor, n_verts: int) -> "MeshTopology":
        """The topology of `faces`, built on first use and remembered on the tensor OBJECT until it is modified in place (as
        producers._check_faces: not keyed on the data pointer, which the caching allocator hands to the next tensor)."""
        c = getattr(faces, _TOPO_ATTR, None)
        if c is not None and c[0] == faces._version and c[1] == int(n_verts):
            return c[2]
        topo = cls(faces, n_verts)
        try:
            setattr(faces, _TOPO_ATTR, (faces._version, int(n_verts), topo))
        except AttributeError:   # (a tensor subclass with __slots__: rebuilt every call)
            pass
        return topo


class Meshes:
    """pytorch3d.structures.Meshes for ONE mesh, with what refine.py:681-706 and sugar_model.py:568-576 read.  Textures are
    accepted and kept, not used."""

    def __init__(self, verts, faces, textures=None):
        if len(verts) != 1 or len(faces) != 1:
            raise NotImplementedError("gaustar_amd.meshes.Meshes holds exactly one mesh")
        self._verts, self._faces = verts[0], faces[0]
        if self._verts.dim() != 2 or self._verts.size(1) != 3:
            raise RuntimeError(f"verts must have dimensions (V, 3), got {tuple(self._verts.shape)}")
        self.textures = textures

    def verts_packed(self) -> torch.Tensor:
        return self._verts

    def faces_packed(self) -> torch.Tensor:
        return self._faces

    def verts_list(self):
        return [self._verts]

    def faces_list(self):
        return [self._faces]

    @property
    def device(self):
        return self._verts.device

    def topology(self) -> MeshTopology:
        return MeshTopology.of(self._faces, int(self._verts.size(0)))

    def edges_packed(self) -> torch.Tensor:
        return self.topology().edges_packed

    def faces_packed_to_edges_packed(self) -> torch.Tensor:
        return self.topology().face_to_edge

    def faces_areas_packed(self) -> torch.Tensor:
        """0.5 |(v1 - v0) x (v2 - v0)| per face, differentiable (torch operations: d|c|/dc = 0 at c = 0)."""
        fv = self._verts[self._faces.long()]
        return 0.5 * torch.linalg.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1).norm(dim=1)


def mesh_normal_consistency(meshes: Meshes) -> torch.Tensor:
    """pytorch3d.loss.mesh_normal_consistency of one mesh: the mean over all pairs of faces sharing an edge of
    1 - cos(n0, n1) (include/gsr.h), 0 for a mesh without such pairs.  One fused HIP op each way
    (losses.surface_mesh_loss with only the normal-consistency term)."""
    from . import losses
    return losses.surface_mesh_loss(meshes.verts_packed(), meshes.topology(), 1.0)


def mesh_laplacian_smoothing(meshes: Meshes, method: str = "uniform") -> torch.Tensor:
    """pytorch3d.loss.mesh_laplacian_smoothing of one mesh: the mean over the vertices of |L v| with the uniform, cotangent or
    cotangent-curvature Laplacian (include/gsr.h restates the rules; parity with pytorch3d itself is not pinned), the weights
    constants.  One fused HIP op each way (losses.mesh_smoothness_loss with only the Laplacian term)."""
    from . import losses
    return losses.mesh_smoothness_loss(meshes.verts_packed(), meshes.topology(), 1.0, method)


__all__ = ["MeshTopology", "Meshes", "mesh_laplacian_smoothing", "mesh_normal_consistency"]
