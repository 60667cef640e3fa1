"""CPU: the cases of tests/producers_cases.py are what they claim to be, before any GPU sees them -- every branch of
matrix_to_unit_quaternion is reached, no case sits on a clamp, the float32 yardstick is finite -- and frame_backward's rule
for the face normal is pinned against float64 autograd in numpy."""
import collections

import numpy as np
import pytest
import torch

import producers_cases as pc
from oracle import producers_oracle as po

COMBOS = [(G, loose) for G in pc.G_VALUES for loose in (False, True)]


def test_case_counts_per_family():
    """No case can drop out unnoticed."""
    count = collections.Counter(c.family for c in pc.all_cases())
    assert dict(count) == pc.FAMILY_COUNTS
    for loose in (False, True):
        got = sorted(c.name for k in pc.BATCHES for c in pc.batch_cases(k, loose))
        assert got == sorted(c.name for c in pc.all_cases() if loose or not c.loose_only)
    assert all(1 <= len(c.faces) <= 8 and c.subject.any() for c in pc.all_cases())
    assert len({(c.family, c.name) for c in pc.all_cases()}) == len(pc.all_cases())


def test_ladders_straddle_the_normal_clamp_and_keep_off_it():
    below = collections.Counter()
    for c in pc.all_cases():
        if c.family not in ("ladder", "sliver"):
            continue
        n = pc.face_cross_norms(c.verts, c.faces)[c.subject]
        assert (np.abs(n / pc.NORMAL_CLAMP - 1) > 0.1).all(), (c.name, n)
        assert (n > 0.4 * c.target).all() and (n < 2.5 * c.target).all(), (c.name, n, c.target)
        assert len({bool(x) for x in n > pc.NORMAL_CLAMP}) == 1, c.name            # a rung is on one side
        below[c.family] += int(n[0] <= pc.NORMAL_CLAMP)
        # the healthy faces hinged on a sliver are healthy
        assert (pc.face_cross_norms(c.verts, c.faces)[~c.subject] > 1e-3).all()
    assert below == {"ladder": 12, "sliver": 4}     # origin: 5e-7 ... 1e-14, offset: 5e-7, 1e-8, two shapes each; slivers 1e-4, 1e-5


def test_degenerate_faces_are_exactly_degenerate():
    for c in pc.all_cases():
        if c.family == "degenerate":
            assert (pc.face_cross_norms(c.verts.astype(np.float32), c.faces)[c.subject] == 0).all()
            assert (pc.face_cross_norms(c.verts, c.faces)[~c.subject] > 1e-2).all()
            shared = set(c.faces[~c.subject].ravel())
            assert set(c.faces[c.subject].ravel()) <= shared            # hinged on healthy faces through every vertex
    v0v1 = next(c for c in pc.all_cases() if c.name == "v0==v1")
    assert (v0v1.verts[0] == v0v1.verts[1]).all() and (v0v1.verts[0] != v0v1.verts[2]).any()


def test_scale_cases_keep_off_the_bounds():
    for G, loose in COMBOS:
        b = pc.make_batch("clamped", G, loose)
        e = torch.exp(b.t["raw_scales"].double())
        for bnd in (pc.LO, pc.HI):
            assert float((e / bnd - 1).abs().min()) > 0.005
    sc = [c for c in pc.all_cases() if c.family == "scales" and c.exp_scale is not None]
    assert sorted(round(c.exp_scale / (pc.LO if "min" in c.name else pc.HI), 2) for c in sc) == [0.5, 0.5, 0.99, 0.99, 1.01, 1.01, 2.0, 2.0]


@pytest.mark.parametrize("G,loose", COMBOS)
def test_float32_and_float64_take_the_same_side_of_every_clamp(G, loose):
    for kind in pc.BATCHES:
        b = pc.make_batch(kind, G, loose)
        (s32, n32), (s64, n64) = pc.masks(b, torch.float32), pc.masks(b, torch.float64)
        assert torch.equal(s32, s64) and torch.equal(n32, n64)
        if kind == "clamped":
            assert bool(s64.any()) and not bool(s64.all()) and bool(n64.any()) and not bool(n64.all())
        _, r64, r32, _ = pc.reference(kind, G, loose)
        q32, q64 = pc.q_abs_of(pc.oracle_R(b, torch.float32)), pc.q_abs_of(r64["R"])
        keep = ~pc.make_batch(kind, G, loose).subject_gaussians()
        top = q64.topk(2, dim=-1).values
        clear = keep & (top[:, 0] - top[:, 1] > 1e-3)
        assert torch.equal(q32.argmax(-1)[clear], q64.argmax(-1)[clear])


def test_every_quaternion_candidate_a_tie_and_a_half_turn_are_reached():
    """Over the axis-aligned family, strict and loose: each best = 0, 1, 2, 3 of matrix_to_unit_quaternion, exact ties of the
    largest q_abs, and half turns (t0 = 0: the case a kernel that always takes candidate 0 gets wrong)."""
    best, ties, half = collections.Counter(), 0, 0
    for loose in (False, True):
        b, r64, _, _ = pc.reference("clamped", 6, loose)
        R32 = pc.oracle_R(b, torch.float32)
        for i, c in enumerate(b.cases):
            if c.family != "branches":
                continue
            g0, g1 = b.grange(i)
            R = r64["R"][g0:g1]
            assert bool(((R == 0) | (R.abs() == 1)).all())              # exact signed permutations
            assert torch.equal(R, R32[g0:g1].double())                  # ... in float32 too
            qa = pc.q_abs_of(R)
            top = qa.topk(2, dim=-1).values
            best.update(qa.argmax(-1).tolist())
            ties += int((top[:, 0] == top[:, 1]).sum())
            half += int((qa[:, 0] == 0).sum())
    print("branches: best", dict(best), "ties", ties, "half turns", half)
    assert dict(best) == BRANCH_COUNTS["best"] and ties == BRANCH_COUNTS["ties"] and half == BRANCH_COUNTS["half"]


BRANCH_COUNTS = {"best": {0: 102, 1: 34, 2: 6, 3: 2}, "ties": 120, "half": 42}   # of 144 Gaussians: G = 6, strict and loose


def test_frames_family_is_smooth_and_about_200_gaussians():
    for G, loose in COMBOS:
        b = pc.make_batch("frames", G, loose)
        assert float(pc.q_abs_gap(b).min()) > 1e-3
    assert pc.make_batch("frames", 6, True).t["raw_complex"].shape[0] == 240


@pytest.mark.parametrize("G,loose", COMBOS)
def test_every_healthy_case_is_finite_and_e32_is_small(G, loose):
    """Finite in float64 and in float32 outside the degenerate cases; prints the yardstick e32 per family and tensor."""
    worst = collections.defaultdict(float)
    for kind in pc.BATCHES:
        b, r64, r32, e32 = pc.reference(kind, G, loose)
        live = ~b.subject_gaussians()
        vlive = torch.ones(b.t["verts"].size(0), dtype=torch.bool)
        for i, c in enumerate(b.cases):
            if c.degenerate:
                vlive[b.vrange[i][0]:b.vrange[i][1]] = False
        for r in (r64, r32):
            for t in (r["points"], r["scaling"], r["quats"], *(g for k, g in r["grads"].items() if k != "verts")):
                assert bool(torch.isfinite(t[live]).all())
            assert bool(torch.isfinite(r["grads"]["verts"][vlive]).all())
        pc.check_points_and_scales(b, r32, r64)                  # the float32 oracle itself meets the fixed bounds
        for (i, k), e in e32.items():
            assert np.isfinite(e), (b.cases[i].name, k)
            worst[(b.cases[i].family, k)] = max(worst[(b.cases[i].family, k)], e)
    for (fam, k), e in sorted(worst.items()):
        print(f"G={G} loose={loose} e32 {fam:10s} {k:12s} {e:.3e}")
        assert e < 1e-2, (fam, k, e)     # (cancellation in a sliver's cross product is the largest; nothing is lost outright)


def _r0_rule_errors(rule):
    """{case name: error of the emulated rule against float64 autograd of the oracle's R_0, normalised by the largest true
    vertex gradient} over the ladder and sliver subject faces."""
    out = {}
    g = np.array([0.3, -0.7, 0.5])
    for c in pc.all_cases():
        if c.family not in ("ladder", "sliver"):
            continue
        f = int(np.nonzero(c.subject)[0][0])
        fv = torch.from_numpy(c.verts.astype(np.float64)[c.faces[f]]).requires_grad_(True)
        R0 = torch.nn.functional.normalize(po.face_normals(fv, torch.tensor([[0, 1, 2]])), dim=-1)
        (R0[0] * torch.from_numpy(g)).sum().backward()
        want = fv.grad.numpy()
        got = pc.r0_vertex_grads(fv.detach().numpy(), g, rule)
        below = pc.face_cross_norms(c.verts, c.faces)[f] <= pc.NORMAL_CLAMP
        out[(c.family, c.name)] = (np.abs(got - want).max() / np.abs(want).max(), below)
    return out


def test_single_normalisation_rule_fails_below_the_clamp_and_the_double_rule_holds():
    """frame_backward used to push dL/dR0 through ONE normalisation with eps 1e-6: 1e6 g below the clamp, no projection and
    the wrong scale.  R0 = normalize(n / max(|n|, 1e-6)) is two, and stays a unit vector down to |n| = 1e-18."""
    old, new = _r0_rule_errors("single"), _r0_rule_errors("double")
    assert sum(b for _, b in old.values()) == 16
    for k in old:
        print(k, f"|n| {'<=' if old[k][1] else '>'} 1e-6: single {old[k][0]:.2e}, double {new[k][0]:.2e}")
        assert new[k][0] < 1e-9, k
        if old[k][1]:
            assert old[k][0] > 0.1, k        # of the order of the gradient itself
        else:
            assert old[k][0] < 1e-9, k
