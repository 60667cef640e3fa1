"""CPU: the definitions of the mesh Laplacian-smoothing loss and the small-area regulariser (include/gsr.h), checked on their
plain-torch restatement (tests/mesh_lap_ref.py) -- closed forms on the regular tetrahedron, the hand-written gradient formula
against autograd -- and the Python surface of the fused op that needs no GPU."""
import math

import pytest
import torch

import mesh_lap_ref as ml
import mesh_reg_ref as mr
from gaustar_amd.losses import mesh_smoothness_loss          # noqa: F401  (the op these definitions are the contract of)
from gaustar_amd.meshes import mesh_laplacian_smoothing      # noqa: F401

MESHES = {"icosphere2": lambda: mr.icosphere(2, noise=0.2), "grid": lambda: mr.grid(6, noise=0.05),
          "non_manifold": mr.non_manifold, "degenerate": mr.degenerate}
# the regular tetrahedron (+-1, +-1, +-1), edge 2 sqrt(2): every vertex is at distance sqrt(3) from the centroid of the whole
# mesh, which is the origin.  uniform: l_i = mean of the other three - v_i = -4/3 v_i, |l_i| = 4 sqrt(3) / 3; cot: equal weights,
# the same l_i; cotcurv: cot 60 = 1 / sqrt(3) on every corner, w_ij = 2 / sqrt(3), S_i = 2 sqrt(3), area 2 sqrt(3) per face,
# a_i = 0.25 / (6 sqrt(3)), l_i = a_i S_i (-4/3 v_i) = -v_i / 9, |l_i| = sqrt(3) / 9
TETRAHEDRON = {"uniform": 4.0 * math.sqrt(3.0) / 3.0, "cot": 4.0 * math.sqrt(3.0) / 3.0, "cotcurv": math.sqrt(3.0) / 9.0}


def _mesh(mk):
    v, f = mk()
    return torch.from_numpy(v), torch.from_numpy(f)


@pytest.mark.parametrize("method", ml.METHODS)
def test_tetrahedron_closed_forms(method):
    v, f = _mesh(mr.tetrahedron)
    assert abs(float(ml.laplacian_loss(v, f, method)) - TETRAHEDRON[method]) <= 1e-14


@pytest.mark.parametrize("name", sorted(MESHES))
@pytest.mark.parametrize("method", ml.METHODS)
def test_gradient_formula_equals_autograd(method, name):
    v, f = _mesh(MESHES[name])
    _, g = ml.smoothness(v, f, 1.0, method)
    h = ml.laplacian_grad(v, f, method)
    assert torch.isfinite(g).all()
    assert float((g - h).abs().max()) <= 1e-12 * max(float(g.abs().max()), 1.0)


@pytest.mark.parametrize("lo", [0.5, 0.1])
def test_area_reg_gradient_formula_equals_autograd(lo):
    v, f = _mesh(MESHES["icosphere2"])
    v = v * torch.linspace(lo, 2.0, v.shape[0], dtype=v.dtype)[:, None]    # uneven faces: some below half the mean area
    loss, g = ml.smoothness(v, f, 0.0, "uniform", 1.0)
    assert float(loss) > 0.0
    h = ml.area_reg_grad(v, f)
    assert float((g - h).abs().max()) <= 1e-12 * max(float(g.abs().max()), 1.0)


def test_area_reg_is_inf_on_a_zero_area_face_and_zero_on_an_even_grid():
    v, f = _mesh(mr.degenerate)
    assert [0, 1, 7] in f.tolist()                      # three collinear vertices
    assert float(ml.area_reg_loss(v, f)) == math.inf
    assert torch.isfinite(ml.area_reg_grad(v, f)).all()
    v, f = _mesh(lambda: mr.grid(6, noise=0.05))
    assert float(ml.area_reg_loss(v, f)) == 0.0


def test_unreferenced_vertex():
    """Vertex 6 has no edge: l = -v, u = -v / |v|, d = -1, so its gradient is (1 / V) d u = (1 / V) v / |v| -- the gradient of
    |v| / V, which pulls the vertex to the origin; cotcurv gives it a_i = 0, l = 0 and no gradient at all."""
    v, f = _mesh(mr.non_manifold)
    V = v.shape[0]
    want = v[6] / v[6].norm() / V
    for method in ("uniform", "cot"):
        assert torch.allclose(ml.laplacian_grad(v, f, method)[6], want, rtol=0, atol=1e-15)
    assert torch.equal(ml.laplacian_grad(v, f, "cotcurv")[6], torch.zeros(3, dtype=v.dtype))


def test_unknown_method_raises_value_error():
    from gaustar_amd import losses, meshes
    v, f = _mesh(mr.tetrahedron)
    topo = meshes.MeshTopology.of(f, 4)
    with pytest.raises(ValueError, match="Method should be one of {uniform, cot, cotcurv}"):
        losses.mesh_smoothness_loss(v.float(), topo, 1.0, "cotan")
    with pytest.raises(ValueError):
        ml.laplacian_loss(v, f, "cotan")


def test_cpu_vertices_raise():
    from gaustar_amd import losses, meshes
    v, f = _mesh(mr.tetrahedron)
    topo = meshes.MeshTopology.of(f, 4)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        losses.mesh_smoothness_loss(v.float(), topo)
    with pytest.raises(RuntimeError, match="there is no CPU path"):
        meshes.mesh_laplacian_smoothing(meshes.Meshes([v.float()], [f]), "cot")


def test_shim_name_is_exported():
    from gaustar_amd import meshes
    from gaustar_amd.meshes import mesh_laplacian_smoothing   # noqa: F401
    assert "mesh_laplacian_smoothing" in meshes.__all__
