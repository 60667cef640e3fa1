"""gaustar_amd.meshes.MeshTopology on the CPU: pytorch3d's edge order and face-to-edge map (restated in mesh_reg_ref.py),
the face pairs of every edge and the vertex-major incidence list the fused regulariser kernels walk."""
import pytest
import torch

import mesh_reg_ref as mr
from gaustar_amd import meshes

MESHES = {**mr.TOPOLOGY_MESHES, "icosphere4": lambda: mr.icosphere(4), "degenerate": mr.degenerate}


def _topo(name):
    v, f = MESHES[name]()
    faces = torch.from_numpy(f)
    return v, faces, meshes.MeshTopology(faces, len(v))


@pytest.mark.parametrize("name", sorted(MESHES))
def test_edges_match_pytorch3d_order(name):
    v, faces, t = _topo(name)
    edges, f2e = mr.p3d_edges(faces, len(v))
    assert torch.equal(t.edges_packed, edges)
    assert torch.equal(t.face_to_edge, f2e)
    assert torch.equal(t.edges.long(), edges) and t.edges.dtype == torch.int32
    # [f, k] is the edge opposite corner k
    for k in range(3):
        a, b = faces[:, (k + 1) % 3], faces[:, (k + 2) % 3]
        assert torch.equal(edges[f2e[:, k]], torch.stack([torch.minimum(a, b), torch.maximum(a, b)], 1))


@pytest.mark.parametrize("name", sorted(MESHES))
def test_pairs(name):
    v, faces, t = _topo(name)
    n = torch.bincount(t.face_to_edge.reshape(-1), minlength=t.E)
    assert t.Q == int((n * (n - 1) // 2).sum())
    idx = mr.p3d_pair_index(faces, len(v))
    assert t.Q == (0 if idx is None else idx[2].shape[0])
    p = t.pairs.long()
    assert p.shape == (t.Q, 4) and t.pairs.dtype == torch.int32
    assert torch.equal(p[:, :2], t.edges_packed[t.pair_edge])
    # a and b are corners of two DIFFERENT faces containing the edge, neither on the edge
    fs = {tuple(sorted(x)) for x in faces.tolist()}
    seen = set()
    for q, (e0, e1, a, b) in enumerate(p.tolist()):
        assert a not in (e0, e1) and b not in (e0, e1)
        assert tuple(sorted([e0, e1, a])) in fs and tuple(sorted([e0, e1, b])) in fs
        seen.add(int(t.pair_edge[q]))
    assert seen == set(torch.nonzero(n >= 2).flatten().tolist())
    # same (edge, opposite corners) multiset as pytorch3d's pairing
    if idx is not None:
        edge_idx, vert_idx, pair_idx = idx
        E = t.edges_packed
        opp = lambda i: [x for x in vert_idx[i].tolist() if x not in E[edge_idx[i]].tolist()][0]
        ref = sorted((int(edge_idx[i]), *sorted((opp(i), opp(j)))) for i, j in pair_idx.tolist())
        got = sorted((int(t.pair_edge[q]), *sorted((a, b))) for q, (_, _, a, b) in enumerate(p.tolist()))
        assert ref == got


@pytest.mark.parametrize("name", sorted(MESHES))
def test_incidence_list_lists_every_incidence_once(name):
    v, faces, t = _topo(name)
    V, Q, E, F = len(v), t.Q, t.E, t.F
    off, ent = t.csr_offsets.long(), t.csr_entries.long()
    assert off.shape == (V + 1,) and int(off[0]) == 0 and int(off[-1]) == ent.numel() == 4 * Q + 2 * E + 3 * F
    assert bool((off[1:] >= off[:-1]).all())
    expect = []
    for q, row in enumerate(t.pairs.tolist()):
        expect += [(row[r], 4 * q + r) for r in range(4)]
    for e, row in enumerate(t.edges_packed.tolist()):
        expect += [(row[r], 4 * (Q + e) + r) for r in range(2)]
    for f, row in enumerate(faces.tolist()):
        expect += [(row[r], 4 * (Q + E + f) + r) for r in range(3)]
    got = []
    for vv in range(V):
        lst = ent[off[vv]:off[vv + 1]].tolist()
        assert lst == sorted(lst)                      # a fixed order: by element, then role
        got += [(vv, c) for c in lst]
    assert sorted(got) == sorted(expect) and len(set(got)) == len(got)


def test_unreferenced_vertex_has_an_empty_list():
    v, faces, t = _topo("non_manifold")
    assert int(t.csr_offsets[7]) == int(t.csr_offsets[6])   # vertex 6 belongs to no face


def test_non_manifold_edge_has_three_pairs():
    v, faces, t = _topo("non_manifold")
    e01 = int(((t.edges_packed[:, 0] == 0) & (t.edges_packed[:, 1] == 1)).nonzero())
    assert int((t.pair_edge == e01).sum()) == 3


def test_topology_cached_per_tensor_and_version():
    v, f = mr.icosphere(1)
    faces = torch.from_numpy(f)
    t1 = meshes.MeshTopology.of(faces, len(v))
    assert meshes.MeshTopology.of(faces, len(v)) is t1
    with torch.no_grad():
        faces[0] = faces[0].flip(0)
    assert meshes.MeshTopology.of(faces, len(v)) is not t1


def test_meshes_shim_cpu_parts():
    v, f = mr.icosphere(1)
    verts = torch.from_numpy(v).requires_grad_(True)
    faces = torch.from_numpy(f)
    m = meshes.Meshes(verts=[verts], faces=[faces])
    assert m.verts_packed() is verts and m.faces_packed() is faces
    assert m.verts_list()[0] is verts and m.faces_list()[0] is faces
    edges, f2e = mr.p3d_edges(faces, len(v))
    assert torch.equal(m.edges_packed(), edges) and torch.equal(m.faces_packed_to_edges_packed(), f2e)
    a = m.faces_areas_packed()
    ref = mr.ref_terms(verts, faces, ref_area=torch.zeros(len(f), dtype=torch.float64))["area"]
    assert torch.allclose(a.mean(), ref)
    a.sum().backward()
    assert verts.grad is not None and torch.isfinite(verts.grad).all()
    with pytest.raises(NotImplementedError):
        meshes.Meshes(verts=[verts, verts], faces=[faces, faces])


def test_faces_out_of_range_raise():
    with pytest.raises(IndexError):
        meshes.MeshTopology(torch.tensor([[0, 1, 5]]), 3)


def test_surface_mesh_loss_has_no_cpu_path():
    from gaustar_amd import losses
    v, f = mr.tetrahedron()
    t = meshes.MeshTopology(torch.from_numpy(f), 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        losses.surface_mesh_loss(torch.from_numpy(v).float(), t, 1.0)


def test_closed_form_meshes_restated_in_f64():
    """The closed forms the GPU test holds the kernels to, checked on the restatement itself."""
    for name, (mk, want) in mr.CLOSED_FORM_NC.items():
        v, f = mk()
        got = float(mr.p3d_normal_consistency(torch.from_numpy(v), torch.from_numpy(f)))
        assert abs(got - want) < 1e-12, (name, got, want)
