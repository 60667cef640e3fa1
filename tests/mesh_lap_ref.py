"""Plain-torch restatement of the mesh Laplacian-smoothing loss and the small-area regulariser as include/gsr.h defines them
(after pytorch3d.loss.mesh_laplacian_smoothing and pytorch3d.ops.laplacian / cot_laplacian, which are not installed here:
parity with pytorch3d itself is not pinned), in any dtype and on any device, through autograd -- and a second, hand-written
evaluation of the gradient formula without autograd.  Shared by tests/test_mesh_lap.py (CPU) and tests/test_gpu_mesh_lap.py."""
import torch

import mesh_reg_ref as mr   # noqa: F401  (the meshes: tetrahedron, grid, non_manifold, degenerate, icosphere)

METHODS = ("uniform", "cot", "cotcurv")


def directed_edges(faces, V):
    """Every edge of the mesh once per direction: (i, j) int64, from mesh_reg_ref.p3d_edges."""
    e, _ = mr.p3d_edges(faces, V)
    return torch.cat([e[:, 0], e[:, 1]]), torch.cat([e[:, 1], e[:, 0]])


def cot_weights(verts, faces):
    """-> (i, j, w) over the directed face-edges (six per face; w_ij is their sum over equal (i, j)) and (face areas [F], by
    Heron's formula clamped at 1e-12 under the root).  Constants: computed on detached positions."""
    v = verts.detach()
    a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
    A = (v[b] - v[c]).norm(dim=1)
    B = (v[a] - v[c]).norm(dim=1)
    C = (v[a] - v[b]).norm(dim=1)
    s = 0.5 * (A + B + C)
    area = (s * (s - A) * (s - B) * (s - C)).clamp(min=1e-12).sqrt()
    A2, B2, C2 = A * A, B * B, C * C
    cota = (B2 + C2 - A2) / area / 4.0
    cotb = (A2 + C2 - B2) / area / 4.0
    cotc = (A2 + B2 - C2) / area / 4.0
    i = torch.cat([b, c, c, a, a, b])
    j = torch.cat([c, b, a, c, b, a])
    w = torch.cat([cota, cota, cotb, cotb, cotc, cotc])
    return i, j, w, area


def _constants(verts, faces, method):
    """-> (i, j, W_ij over directed (i, j) entries, c [V], d [V]) with l_i = c_i sum_j W_ij v_j + d_i v_i."""
    V = verts.shape[0]
    zeros = torch.zeros(V, dtype=verts.dtype, device=verts.device)
    if method == "uniform":
        i, j = directed_edges(faces, V)
        deg = zeros.index_add(0, i, torch.ones_like(i, dtype=verts.dtype))
        W = torch.where(deg[i] > 0, 1.0 / deg[i], deg[i])
        return i, j, W, torch.ones_like(zeros), -torch.ones_like(zeros)
    if method not in ("cot", "cotcurv"):
        raise ValueError("Method should be one of {uniform, cot, cotcurv}")
    i, j, w, area = cot_weights(verts, faces)
    S = zeros.index_add(0, i, w)
    if method == "cot":
        n = torch.where(S > 0, 1.0 / S, S)
        return i, j, w, n, -torch.ones_like(zeros)
    va = zeros.index_add(0, faces.reshape(-1), area.repeat_interleave(3))
    a = torch.where(va > 0, 0.25 / va, torch.zeros_like(va))
    return i, j, w, a, -a * S


def laplacian_loss(verts, faces, method="uniform"):
    """(1 / V) sum_i |l_i|, differentiable w.r.t. verts; the weights are constants."""
    i, j, W, c, d = _constants(verts, faces, method)
    gathered = torch.zeros_like(verts).index_add(0, i, W[:, None] * verts[j])
    l = c[:, None] * gathered + d[:, None] * verts
    return l.norm(dim=1).sum() / verts.shape[0]


def laplacian_grad(verts, faces, method="uniform"):
    """d laplacian_loss / d verts by the formula, no autograd: (1 / V) (sum_i c_i W_ik u_i + d_k u_k), u = l / |l| (0 at 0)."""
    v = verts.detach()
    i, j, W, c, d = _constants(v, faces, method)
    gathered = torch.zeros_like(v).index_add(0, i, W[:, None] * v[j])
    l = c[:, None] * gathered + d[:, None] * v
    n = l.norm(dim=1, keepdim=True)
    u = torch.where(n > 0, l / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(l))
    g = torch.zeros_like(v).index_add(0, j, (c[i] * W)[:, None] * u[i])      # row i of W scatters to its columns
    return (g + d[:, None] * u) / v.shape[0]


def face_areas(verts, faces):
    fv = verts[faces]
    return 0.5 * torch.linalg.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1).norm(dim=1)


def area_reg_loss(verts, faces):
    """refine.py:713-718: relu(mean_area / face_area - 2).mean(), the mean area under no_grad."""
    area = face_areas(verts, faces)
    with torch.no_grad():
        m = area.mean()
    return torch.relu(m / area - 2.0).mean()


def area_reg_grad(verts, faces):
    """d area_reg_loss / d verts by the formula: a face with m / area > 2 gives -(1 / F) m / area^2 d area / d v; a face of area
    exactly 0 gives 0 (the stated departure from torch's NaN)."""
    v = verts.detach()
    F = faces.shape[0]
    p0, p1, p2 = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    u, w = p1 - p0, p2 - p0
    cr = torch.linalg.cross(u, w, dim=1)
    ln = cr.norm(dim=1)
    area = 0.5 * ln
    m = area.mean()
    ok = area > 0
    safe = torch.where(ok, area, torch.ones_like(area))
    on = ok & (m / safe > 2.0)
    coef = torch.where(on, -(m / (safe * safe)) / F, torch.zeros_like(area))
    gc = (0.5 * coef / torch.where(ok, ln, torch.ones_like(ln)))[:, None] * cr
    gu, gw = torch.linalg.cross(w, gc, dim=1), torch.linalg.cross(gc, u, dim=1)
    g = torch.zeros_like(v)
    g = g.index_add(0, faces[:, 1], gu).index_add(0, faces[:, 2], gw).index_add(0, faces[:, 0], -(gu + gw))
    return g


def smoothness(verts, faces, laplacian_factor=1.0, method="uniform", area_reg_factor=0.0):
    """-> (loss, gradient) of the composition through autograd, on a fresh leaf of `verts`."""
    x = verts.detach().clone().requires_grad_(True)
    loss = x.sum() * 0.0
    if laplacian_factor != 0.0:
        loss = loss + laplacian_factor * laplacian_loss(x, faces, method)
    if area_reg_factor != 0.0:
        loss = loss + area_reg_factor * area_reg_loss(x, faces)
    loss.backward()
    return loss.detach(), x.grad
