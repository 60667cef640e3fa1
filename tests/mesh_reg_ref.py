"""Restatements of pytorch3d's mesh algorithms in plain torch (pytorch3d itself is not installed), and the small meshes the
mesh-regulariser tests use.  Shared by tests/test_mesh_topology.py (CPU) and tests/test_gpu_mesh_reg.py (GPU)."""
import math

import numpy as np
import torch

from gaustar_amd import scene


def p3d_edges(faces: torch.Tensor, V: int):
    """Meshes._compute_edges_packed for one mesh: -> (edges_packed [E,2], faces_packed_to_edges_packed [F,3])."""
    F = faces.shape[0]
    v0, v1, v2 = faces.chunk(3, dim=1)
    e01 = torch.cat([v0, v1], dim=1)
    e12 = torch.cat([v1, v2], dim=1)
    e20 = torch.cat([v2, v0], dim=1)
    edges = torch.cat([e12, e20, e01], dim=0)
    edges, _ = edges.sort(dim=1)
    edges_hash = V * edges[:, 0] + edges[:, 1]
    u, inverse_idxs = torch.unique(edges_hash, return_inverse=True)
    edges_packed = torch.stack([u // V, u % V], dim=1)
    face_to_edge = inverse_idxs[torch.arange(3 * F, device=faces.device).view(3, F).t()]
    return edges_packed, face_to_edge


def p3d_pair_index(faces: torch.Tensor, V: int):
    """The no-grad half of pytorch3d.loss.mesh_normal_consistency: (edge_idx, vert_idx, vert_edge_pair_idx) or None."""
    F = faces.shape[0]
    _edges, face_to_edge = p3d_edges(faces, V)
    edge_idx = face_to_edge.reshape(F * 3)
    vert_idx = faces.view(1, F, 3).expand(3, F, 3).transpose(0, 1).reshape(3 * F, 3)
    edge_idx, edge_sort_idx = edge_idx.sort(stable=True)
    vert_idx = vert_idx[edge_sort_idx]
    E = _edges.shape[0]
    edge_num = edge_idx.bincount(minlength=E)
    if bool((edge_num == 2).all()):   # a closed manifold: each edge's one pair, [[0, 1], [2, 3], ...] (no Python loop)
        return edge_idx, vert_idx, torch.arange(2 * E, device=faces.device).view(E, 2)
    lists, k = [], 0
    for n in edge_num.tolist():
        lists.append(list(range(k, k + n)))
        k += n
    pairs = [torch.combinations(torch.tensor(x, device=faces.device), 2) for x in lists if len(x) > 1]
    if not pairs:
        return None
    return edge_idx, vert_idx, torch.cat(pairs, dim=0)


def p3d_normal_consistency(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """pytorch3d.loss.mesh_normal_consistency of one mesh, differentiable w.r.t. verts (any dtype)."""
    V = verts.shape[0]
    edges_packed, _ = p3d_edges(faces, V)
    idx = p3d_pair_index(faces, V)
    if idx is None:
        return verts.sum() * 0.0
    edge_idx, vert_idx, pair_idx = idx
    v0 = verts[edges_packed[edge_idx, 0]]
    v1 = verts[edges_packed[edge_idx, 1]]
    n_temp0 = torch.linalg.cross(v1 - v0, verts[vert_idx[:, 0]] - v0, dim=1)
    n_temp1 = torch.linalg.cross(v1 - v0, verts[vert_idx[:, 1]] - v0, dim=1)
    n_temp2 = torch.linalg.cross(v1 - v0, verts[vert_idx[:, 2]] - v0, dim=1)
    n = n_temp0 + n_temp1 + n_temp2
    n0 = n[pair_idx[:, 0]]
    n1 = -n[pair_idx[:, 1]]
    loss = 1 - torch.nn.functional.cosine_similarity(n0, n1, dim=1)
    return loss.sum() / pair_idx.shape[0]


def ref_terms(verts, faces, ref_edge_len=None, ref_area=None):
    """refine.py:690-702's edge and area terms (without their factors) over p3d_edges / face areas."""
    edges_packed, _ = p3d_edges(faces, verts.shape[0])
    out = {}
    if ref_edge_len is not None:
        ve = verts[edges_packed]
        out["edge"] = (((ve[:, 0] - ve[:, 1]).norm(dim=1, p=2) - ref_edge_len) ** 2).mean()
    if ref_area is not None:
        fv = verts[faces]
        area = 0.5 * torch.linalg.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1).norm(dim=1)
        out["area"] = (area - ref_area).abs().mean()
    return out


# ---------------------------------------------------------------------------------------------------------------- meshes
def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64)
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int64)
    return v, f


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)
    return v, f


def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)   # index = 4x + 2y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = []
    for a, b, c, d in quads:
        f += [[a, b, c], [a, c, d]]
    return v, np.array(f, np.int64)


def grid(n=4, noise=0.0, seed=0):
    """An open (n+1) x (n+1) grid in the z = 0 plane, two triangles per cell (boundary edges)."""
    xs, ys = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size)], 1).astype(np.float64) / n
    if noise:
        v[:, 2] += np.random.default_rng(seed).normal(scale=noise, size=len(v))
    f = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
            f += [[a, b, c], [a, c, d]]
    return v, np.array(f, np.int64)


def non_manifold():
    """Three triangles sharing the edge (0, 1), plus a fourth face on one of them; vertex 6 is referenced by no face."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -0.7, 0.7], [0.4, -0.6, -0.8], [1.2, 1.1, 0.3], [5, 5, 5]], np.float64)
    f = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [1, 5, 2]], np.int64)
    return v, f


def degenerate():
    """The non-manifold mesh with a zero-area face (three collinear vertices) hinged on a regular one."""
    v, f = non_manifold()
    v = np.vstack([v, [[2, 0, 0]]])
    f = np.vstack([f, [[0, 1, 7], [1, 3, 7]]])
    return v, f


def icosphere(level, noise=0.0, seed=0):
    v, f = scene.icosphere(level)
    v = v.astype(np.float64)
    if noise:
        edge = np.linalg.norm(v[f[:, 0]] - v[f[:, 1]], axis=1).mean()
        v = v + np.random.default_rng(seed).normal(scale=noise * edge, size=v.shape)
    return v, f.astype(np.int64)


CLOSED_FORM_NC = {   # mesh -> normal consistency, from the dihedral angles (1 - cos of the angle between face normals)
    "tetrahedron": (tetrahedron, 4.0 / 3.0),
    "octahedron": (octahedron, 2.0 / 3.0),
    "icosahedron": (lambda: icosphere(0), 1.0 - math.sqrt(5.0) / 3.0),
    "cube": (cube, 2.0 / 3.0),
    "flat_grid": (grid, 0.0),
}

TOPOLOGY_MESHES = {
    "icosphere2": lambda: icosphere(2),
    "grid": lambda: grid(5),
    "non_manifold": non_manifold,
}
