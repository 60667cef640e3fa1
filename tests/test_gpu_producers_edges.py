"""GPU: the mesh-bound Gaussian producer (gsr_mesh_gaussians and its backward) against float64 on small, sliver and
degenerate faces, parameters at their clamps and every branch of the matrix-to-quaternion conversion -- the cases of
tests/producers_cases.py, checked on the CPU by tests/test_producers_cases.py.

Bounds: the kernel's normalised error is at most 4 times that of the float32 CPU oracle (e32) for the same case and tensor -- 32
times for dL_draw_complex and dL_dverts, see producers_cases.EDGE_FACTORS for the operation and the measurement behind it --
or ERR_FLOOR = 8 * 2^-24 where e32 is smaller; points within the rounding of their three products and sums; scales
and the gradient of the raw scales within rtol 2e-6 (__expf) with the clamps taken exactly.  Per-Gaussian tensors are
normalised by the case's largest |reference|, dL_dverts per vertex by the float64 sum of the absolute per-corner contributions
(producers_cases.case_errors).  Every test prints the ratio kernel error / e32 it measured per family and tensor."""
import collections

import numpy as np
import pytest
import torch

import producers_cases as pc
from oracle import producers_oracle as po

pytestmark = pytest.mark.gpu
COMBOS = [(G, loose) for G in pc.G_VALUES for loose in (False, True)]


def _hip(b, **kw):
    from gaustar_amd import producers
    return pc.run(producers.mesh_bound_gaussians, b, dev="cuda", **kw)


def _hold(tag, b, got, r64, e32):
    """Every healthy case and tensor within bound(e32); prints the worst ratio per family and tensor."""
    worst, bad = collections.defaultdict(float), []
    for (i, k), e in pc.case_errors(b, got, r64).items():
        c = b.cases[i]
        ratio = e / max(e32[(i, k)], 1e-300)
        if e > pc.ERR_FLOOR:                                     # (below the floor a ratio says nothing)
            worst[(c.family, k)] = max(worst[(c.family, k)], ratio)
        if not e <= pc.bound(e32[(i, k)], k):
            bad.append(f"{c.family} {c.name} {k}: error {e:.3e}, e32 {e32[(i, k)]:.3e}, ratio {ratio:.2f}")
    for (fam, k), r in sorted(worst.items()):
        print(f"{tag} ratio {fam:10s} {k:12s} {r:.3f}")
    assert not bad, f"{tag}: {len(bad)} over the bound:\n" + "\n".join(bad)


@pytest.mark.parametrize("G,loose", COMBOS)
def test_every_case_against_float64(G, loose, hip_lib):
    """All families, both kernel shapes (G <= 8: a lane per Gaussian; G = 9: a thread per face) on the same faces.  Below the
    normal clamp (ladder and sliver rungs with |e1 x e2| < 1e-6) a backward that takes R0 = normalize(n / max(|n|, 1e-6)) for
    one normalisation is wrong in dL_dverts by the order of the gradient itself; a raw complex number shorter than
    F.normalize's eps (complex 1e-15) makes R no rotation, where the tangent-space shortcut of the backward does not hold."""
    for kind in pc.BATCHES:
        b, r64, _, e32 = pc.reference(kind, G, loose)
        got = _hip(b)
        assert pc.all_finite(got), f"{kind}: a non-finite output or gradient"       # the degenerate faces included
        assert float((got["quats"].norm(dim=-1) - 1).abs().max()) < 1e-6
        pc.check_points_and_scales(b, got, r64)
        _hold(f"G={G} loose={int(loose)} {kind}", b, got, r64, e32)


@pytest.mark.parametrize("G,loose", COMBOS)
def test_loss_on_the_quaternion_itself(G, loose, hip_lib):
    """The backward's header: the tangent-space shortcut is exact for ANY loss on the unit quaternion, not only one that
    reads it through R(q).  sum(w q s) on top of the R(q) loss, s = sign(q_hip . q_ref) per row (q and -q are one rotation),
    on random healthy frames away from a change of candidate, where the oracle is smooth."""
    b, r64, r32, _ = pc.reference("frames", G, loose)
    q_hip = _hip(b)["quats"].double()
    s = torch.sign((q_hip * r64["quats"]).sum(-1))
    s32 = torch.sign((q_hip * r32["quats"].double()).sum(-1))
    assert bool((s.abs() == 1).all()) and bool((s32.abs() == 1).all())
    ref = pc.run_f64(b, q_sign=s)
    e32 = pc.case_errors(b, pc.run(po.mesh_bound_gaussians, b, q_sign=s32), ref)
    got = _hip(b, q_sign=torch.ones_like(s))
    assert pc.all_finite(got)
    _hold(f"G={G} loose={int(loose)} frames, loss on q", b, got, ref, e32)


@pytest.mark.parametrize("G,loose", COMBOS)
def test_a_muted_degenerate_face_leaves_its_neighbours_alone(G, loose, hip_lib):
    """Zero upstream gradient on the Gaussians of a zero-area face (collinear, v0 == v1, all three equal) or of a face whose
    raw complex number is (0, 0): the gradients at the vertices it shares with healthy faces are those of the mesh without
    that face, within the healthy faces' own bound.  0 x 1e12 stays 0 and never becomes NaN."""
    b = pc.make_batch("clamped", G, loose)
    mute = b.subject_gaussians()
    assert int(mute.sum()) == 4 * G
    got = _hip(b, mute=mute)
    assert pc.all_finite(got)
    rest, _ = pc.without_subjects(b)
    r64, r32 = pc.run_f64(rest), pc.run(po.mesh_bound_gaussians, rest)
    n = 0
    for i, c in enumerate(b.cases):
        if not c.degenerate:
            continue
        lo, hi = b.vrange[i]
        e, e32 = pc.vertex_err(got["grads"]["verts"], r64, lo, hi), pc.vertex_err(r32["grads"]["verts"], r64, lo, hi)
        print(f"G={G} loose={int(loose)} muted {c.name}: error {e:.3e}, e32 {e32:.3e}")
        assert e <= pc.bound(e32, "verts"), (c.name, e, e32)
        n += 1
    assert n == 4
    for k in ("raw_complex", "delta_r"):                      # and the muted Gaussians' own gradients are exactly zero
        if k in got["grads"]:
            assert bool((got["grads"][k][mute] == 0).all()), k


def _ulp_distance(a, b):
    def key(t):
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int((key(a) - key(b)).abs().max())


def test_both_kernel_shapes_on_one_model_ulp_report(hip_lib):
    """Information only: the largest ulp distance, on the per-Gaussian outputs, between a G = 6 model (lane per Gaussian)
    and a G = 12 model that repeats its per-face parameters (thread per face).  The comment above dot_zxy claims last-bit
    agreement for the backward."""
    b6 = pc.make_batch("clamped", 6, True)
    F = b6.t["faces"].size(0)
    twice = lambda t: torch.cat([t.reshape(F, 6, -1)] * 2, 1).reshape(F * 12, -1)
    t12 = {k: (twice(v) if k in ("raw_scales", "raw_complex", "delta_t", "delta_r", "wp", "ws", "wq", "wq4") else v)
           for k, v in b6.t.items()}
    t12["bary"] = torch.cat([b6.t["bary"]] * 2)
    b12 = pc.Batch("clamped", 12, True, b6.cases, t12, b6.lo, b6.hi, b6.vrange, b6.frange)
    r6, r12 = _hip(b6), _hip(b12)
    live = ~b6.subject_gaussians()
    first = lambda t: t.reshape(F, 12, -1)[:, :6].reshape(F * 6, -1)
    for name, a, c in [("quaternions", r6["quats"], r12["quats"]), ("points", r6["points"], r12["points"])] + \
                      [(f"dL_d{k}", r6["grads"][k], r12["grads"][k]) for k in ("raw_scales", "raw_complex", "delta_t", "delta_r")]:
        print(f"G=6 against G=12, {name}: {_ulp_distance(a[live], first(c)[live])} ulp")
    assert pc.all_finite(r12)


def test_model_route_on_a_millimetre_sphere(hip_lib):
    """harness.SurfaceGaussians on scene.icosphere(2, 0.003): |e1 x e2| is about 7e-7 on every face, below the normal clamp.
    Gradients of points, scaling and quaternions to `_points` under the R(q) loss against float64; no render involved."""
    from gaustar_amd import harness, scene
    v, f = scene.icosphere(2, 0.003)
    n = pc.face_cross_norms(v.astype(np.float32), f)
    assert (n < 0.9 * pc.NORMAL_CLAMP).all() and (n > 1e-7).all() and len(f) == 320
    dev = torch.device("cuda:0")
    model = harness.SurfaceGaussians(torch.from_numpy(v).float().to(dev), torch.from_numpy(f).long().to(dev), 6,
                                     surface_mesh_thickness=pc.THICKNESS)
    g = torch.Generator().manual_seed(5)
    N = model.n_points
    with torch.no_grad():
        model._quaternions.copy_(torch.randn(N, 2, generator=g).to(dev))
    t = dict(verts=model._points.detach().cpu(), faces=model._surface_mesh_faces.cpu(),
             bary=model.surface_triangle_bary_coords[..., 0].cpu(), raw_scales=model._scales.detach().cpu(),
             raw_complex=model._quaternions.detach().cpu(), delta_t=None, delta_r=None,
             wp=torch.randn(N, 3, generator=g), ws=torch.randn(N, 3, generator=g), wq=torch.randn(N, 3, generator=g),
             W3=torch.randn(3, 3, generator=g), wq4=torch.randn(N, 4, generator=g))
    b = pc.Batch("model", 6, False, [], t, None, None, [(0, len(v))], [(0, len(f))])
    pc.loss_of(b, model.points, model.scaling, model.quaternions).backward()
    got = model._points.grad.cpu()
    r64, r32 = pc.run_f64(b), pc.run(po.mesh_bound_gaussians, b)
    e, e32 = pc.vertex_err(got, r64), pc.vertex_err(r32["grads"]["verts"], r64)
    print(f"model route: dL_d_points error {e:.3e}, e32 {e32:.3e}, ratio {e / e32:.3f}")
    assert bool(torch.isfinite(got).all()) and e <= pc.bound(e32, "verts"), (e, e32)
    np.testing.assert_allclose(model._scales.grad.cpu().numpy(), r64["grads"]["raw_scales"].numpy(), rtol=2e-6, atol=0)
    ek = pc.norm_err(model._quaternions.grad.cpu(), r64["grads"]["raw_complex"])
    assert ek <= pc.bound(pc.norm_err(r32["grads"]["raw_complex"], r64["grads"]["raw_complex"]), "raw_complex"), ek
