"""Hand-built meshes for the mesh-bound Gaussian producer (gsr_mesh_gaussians) and its float64 reference.

A CASE is a mesh of 1 to 8 faces with rules for its per-Gaussian parameters: one shape at one scale with one parameter
setting, so that its rows share a magnitude and an error can be normalised per case.  Cases of one kind are laid side by side
as disjoint components of one mesh (a BATCH) for a launch.  The reference is oracle.producers_oracle.mesh_bound_gaussians in
float64 on the float32-rounded inputs, with autograd; the same function in float32 on the CPU is the yardstick: a kernel may be
EDGE_FACTOR times as far from float64 as it is (FMA contraction, another order of the same float32 operations), or
ERR_FLOOR where it happens to be exact.

tests/test_producers_cases.py checks the cases themselves on the CPU; tests/test_gpu_producers_edges.py holds the kernels to
them."""
import functools
import math
import zlib
from dataclasses import dataclass, field

import numpy as np
import torch

from oracle import producers_oracle as po

EDGE_FACTOR = 4.0            # the factor of tests/test_gpu_losses_edges.py (loss_cases.EDGE_FACTOR)
ERR_FLOOR = 8 * 2.0 ** -24
# dL_draw_complex and dL_dverts take 32 instead of 4.  Measured on the device: rotations stay within 3.3 x e32 and dL_ddelta_r
# within 2.4, these two reach 24.6 and 16.8 with no defect behind it.  The operation: the backward turns dL/dq into the rotation
# vector Gw (the radial part of dL/dq, the larger one under an R(q) loss, cancels) and contracts 1/2 [Gw]x R with the frame; the
# raw complex number only receives Gw . R0, so its gradient carries a rounding of 2^-24 |dL/dq| whatever its own size.  In the
# worst case (branches n-z/270, G = 1: |dL/dq| = 2.7, |Gw| = 1.3, Gw . R0 = 0.0089) the kernel is 1.2e-7 = 0.75 * 2^-24 |dL/dq|
# off, which is 1.4e-5 of that gradient, while the float32 oracle multiplies exact zeros and ones there and is off by 5.7e-7: a
# case of one face is a sample of one, and e32 of a lucky sample is no measure of the conditioning.  32 is below twice either
# measured ratio, and the defects these cases were built for miss by factors of 1e5 and more.
EDGE_FACTORS = {"R": EDGE_FACTOR, "delta_t": EDGE_FACTOR, "delta_r": EDGE_FACTOR, "raw_complex": 32.0, "verts": 32.0}
NORMAL_CLAMP = 1e-6          # pytorch3d's face-normal clamp
THICKNESS = 3e-6
LO, HI = 0.012, 0.03         # min / max Gaussian scale of the clamped batches
G_VALUES = (1, 6, 8, 9)      # 1, 6, 8: lane-per-Gaussian kernels; 9: per-face kernels
BARY6 = [[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3], [1 / 6, 5 / 12, 5 / 12], [5 / 12, 1 / 6, 5 / 12],
         [5 / 12, 5 / 12, 1 / 6]]
FAMILY_COUNTS = {"ladder": 24, "sliver": 10, "degenerate": 3, "complex": 21, "delta_r": 5, "scales": 9, "branches": 12,
                 "frames": 5}
GRAD_NAMES = ("verts", "raw_scales", "raw_complex", "delta_t", "delta_r")


@dataclass
class Case:
    family: str
    name: str
    verts: np.ndarray                       # [V,3] float32
    faces: np.ndarray                       # [F,3] int64
    subject: np.ndarray                     # [F] bool: the faces under study; the others are healthy faces hinged on them
    degenerate: bool = False                # subject faces: no comparison of rotations or of the faces' own gradients
    clamp: bool = True                      # launch with min / max scale
    loose_only: bool = False                # the family has no strict form
    complex_: tuple = None                  # raw_complex of every subject Gaussian
    delta_r: tuple = None                   # delta_r of every subject Gaussian, or a list to cycle through
    exp_scale: float = None                 # exp(raw_scales) of every subject Gaussian
    target: float = None                    # ladder / sliver: the |e1 x e2| aimed at


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))


# ----------------------------------------------------------------------------------------------------------- geometry
_TRI = np.array([[0.0, 0.0, 0.0], [1.0, 0.25, 0.125], [0.25, 1.0, -0.25]])                # |e1 x e2| = 0.99657
_FAN_ANGLES = np.deg2rad([0.0, 70.0, 150.0, 220.0, 300.0])
_FAN = np.concatenate([[[0.0, 0.0, 0.1]], np.stack([np.cos(_FAN_ANGLES), np.sin(_FAN_ANGLES),
                                                    np.array([0.0, 0.2, -0.1, 0.15, 0.05])], -1)])
_FAN_FACES = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5]])
_ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])                 # a rotation with no zero in its way
OFFSET = np.array([0.0, 1.2, 0.0])


def face_cross_norms(verts, faces):
    """|e1 x e2| per face, float64 of the given (float32) vertices."""
    fv = np.asarray(verts, np.float64)[faces]
    return np.linalg.norm(np.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0]), axis=-1)


def _scaled(shape, faces, target, offset):
    """The shape scaled so that its faces' mean |e1 x e2| is `target`, moved to `offset`, rounded to float32."""
    s = math.sqrt(target / face_cross_norms(shape, faces).mean())
    return _f32(shape * s + offset)


def _ladder():
    out = []
    for where, offset, rungs in (("origin", np.zeros(3), (1e-2, 1e-5, 2e-6, 5e-7, 1e-8, 1e-11, 1e-14)),
                                 ("offset", OFFSET, (1e-2, 1e-5, 2e-6, 5e-7, 1e-8))):
        for t in rungs:
            out.append(Case("ladder", f"tri/{where}/{t:g}", _scaled(_TRI, np.array([[0, 1, 2]]), t, offset), np.array([[0, 1, 2]]),
                            np.array([True]), target=t))
            out.append(Case("ladder", f"fan/{where}/{t:g}", _scaled(_FAN, _FAN_FACES, t, offset), _FAN_FACES.copy(),
                            np.ones(4, bool), target=t))
    return out


SLIVER_BASE = 0.0625   # (a base of 0.1 would put the 1e-4 rung at |e1 x e2| = 1e-6, on the clamp itself; 1/16 is exact in float32
                       # and leaves three rungs above the clamp and two below)


def _slivers():
    """Base SLIVER_BASE, height / base 1e-1 ... 1e-5: |e1 x e2| = 3.90625e-3 * ratio.  The sliver (A, B, C) shares both base
    vertices with a healthy face (B, A, D); once in the z = 0 plane at the origin, once turned by _ROT about OFFSET."""
    out = []
    for where, rot, offset in (("plane", np.eye(3), np.zeros(3)), ("turned", _ROT, OFFSET)):
        for k in range(1, 6):
            ratio = 10.0 ** -k
            h = SLIVER_BASE * ratio
            v = np.array([[0.0, 0.0, 0.0], [SLIVER_BASE, 0.0, 0.0], [0.0234375, h, 0.0], [0.03125, -0.046875, 0.015625]])
            out.append(Case("sliver", f"{where}/{ratio:g}", _f32(v @ rot.T + offset), np.array([[0, 1, 2], [1, 0, 3]]),
                            np.array([True, False]), target=SLIVER_BASE * h))
    return out


def _degenerate():
    """Dyadic coordinates: the zero edges and the zero normal are exact in float32.  Each degenerate face (the first) shares
    every one of its vertices with a healthy face."""
    A, B, C, D, E, F_ = [0.5, 1.0, -0.25], [0.75, 1.0, -0.25], [1.0, 1.0, -0.25], [0.75, 1.5, -0.125], [0.25, 1.25, 0.0], [0.5, 0.5, 0.25]
    sub = lambda n: np.array([True] + [False] * (n - 1))
    return [
        Case("degenerate", "collinear", _f32([A, B, C, D]), np.array([[0, 1, 2], [0, 1, 3], [1, 2, 3]]), sub(3), degenerate=True),
        Case("degenerate", "v0==v1", _f32([A, A, D, E, F_]), np.array([[0, 1, 2], [0, 3, 2], [1, 2, 4]]), sub(3), degenerate=True),
        Case("degenerate", "all equal", _f32([A, A, A, D, E, F_]), np.array([[0, 1, 2], [0, 3, 4], [1, 4, 5], [2, 5, 3]]), sub(4),
             degenerate=True),
    ]


_HEALTHY = _f32(_TRI * 0.2 + OFFSET)
_HINGED = (_f32(np.concatenate([_TRI, [[1.0, 1.0, 0.5]]]) * 0.2 + OFFSET), np.array([[0, 1, 2], [2, 1, 3]]))


def _one_face(family, name, **kw):
    return Case(family, name, _HEALTHY.copy(), np.array([[0, 1, 2]]), np.array([True]), **kw)


def _parameters():
    out = [Case("complex", "zero", _HINGED[0].copy(), _HINGED[1].copy(), np.array([True, False]), degenerate=True, complex_=(0.0, 0.0))]
    for m in (1e-15, 1e-6, 1.0, 1e15):                                    # (squares stay normal in float32)
        for nm, d in (("+x", (1, 0)), ("-x", (-1, 0)), ("+y", (0, 1)), ("-y", (0, -1)), ("diag", (0.6, -0.8))):
            out.append(_one_face("complex", f"{m:g}/{nm}", complex_=(m * d[0], m * d[1])))
    base = np.array([0.5, -0.3, 0.7, 0.4])
    base = base / np.linalg.norm(base)
    for nm, q in (("norm 1e-3", 1e-3 * base), ("norm 1", base), ("norm 1e3", 1e3 * base), ("negative real", base * [-1, 1, 1, 1]),
                  ("zero real", np.array([0.0, 0.6, -0.48, 0.64]))):
        out.append(_one_face("delta_r", nm, delta_r=tuple(q), loose_only=True))
    for bound, bn in ((LO, "min"), (HI, "max")):
        for f in (0.5, 0.99, 1.01, 2.0):
            out.append(_one_face("scales", f"{f:g} x {bn}", exp_scale=f * bound))
    out.append(_one_face("scales", "no clamp", clamp=False))
    return out


def _branches():
    """Axis-aligned faces (normal and first edge along coordinate axes) with in-plane quarter turns: every entry of R is
    exactly 0 or +-1 in float32 and float64, so the candidates of matrix_to_unit_quaternion tie exactly where they tie.
    Loose binding multiplies by axis-aligned delta_r (identity and the three half turns, one per Gaussian in turn)."""
    out = []
    P = np.array([0.5, 1.0, -0.25])
    # (v0, v1, v2): normal (v1 - v0) x (v2 - v0), first frame edge v0 - v1
    shapes = {"n-z": [[0.25, 0, 0], [0, 0, 0], [0, 0.25, 0]],
              "n+x": [[0, 0, 0.25], [0, 0, 0], [0, 0.25, 0]],
              "n-y": [[0, 0, 0], [0.25, 0, 0], [0, 0, 0.25]]}
    dr_cycle = [(1.0, 0, 0, 0), (0, 1.0, 0, 0), (0, 0, 1.0, 0), (0, 0, 0, 1.0)]
    for sn, sv in shapes.items():
        for tn, c in (("0", (1.0, 0.0)), ("90", (0.0, 1.0)), ("180", (-1.0, 0.0)), ("270", (0.0, -1.0))):
            out.append(Case("branches", f"{sn}/{tn}", _f32(np.array(sv) + P), np.array([[0, 1, 2]]), np.array([True]), complex_=c,
                            delta_r=dr_cycle))
    return out


def _frames():
    """Random healthy frames (8 faces each, random vertices in a box) for the loss on q itself."""
    out = []
    for i in range(5):
        r = np.random.default_rng(500 + i)
        v = r.uniform(-0.5, 0.5, size=(24, 3)) + OFFSET
        out.append(Case("frames", f"random/{i}", _f32(v), np.arange(24).reshape(8, 3), np.ones(8, bool), clamp=False))
    return out


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(_ladder() + _slivers() + _degenerate() + _parameters() + _branches() + _frames())


BATCHES = ("clamped", "unclamped", "frames")


def batch_cases(kind, loose):
    cs = [c for c in all_cases() if not (c.loose_only and not loose)]
    if kind == "frames":
        return [c for c in cs if c.family == "frames"]
    return [c for c in cs if c.family != "frames" and c.clamp == (kind == "clamped")]


# ----------------------------------------------------------------------------------------------------------- batches
def bary_coords(G):
    if G == 1:
        return _f32([[1 / 3, 1 / 3, 1 / 3]])
    if G == 6:
        return _f32(BARY6)
    b = np.random.default_rng(G).uniform(0.1, 1.0, size=(G, 3))
    return _f32(b / b.sum(-1, keepdims=True))


def _safe_scales(r, n):
    """exp(raw) below, between and above the clamp bounds, never within 10 % of one."""
    u = r.uniform(size=(n, 2))
    lo, mid, hi = LO * (0.3 + 0.6 * u), LO * 1.1 + (HI * 0.9 - LO * 1.1) * u, HI * (1.1 + 1.9 * u)
    pick = r.integers(0, 3, size=(n, 2))
    return np.where(pick == 0, lo, np.where(pick == 1, mid, hi))


def _case_params(c, G, loose):
    r = np.random.default_rng(zlib.crc32(f"{c.family}/{c.name}/{G}/{int(loose)}".encode()))
    F = len(c.faces)
    n = F * G
    sub = np.repeat(c.subject, G)
    es = _safe_scales(r, n) if c.clamp else np.exp(r.normal(-4.0, 0.4, size=(n, 2)))
    if c.exp_scale is not None:
        es[sub] = c.exp_scale
    ang, mag = r.uniform(0, 2 * np.pi, n), r.uniform(0.5, 2.0, n)
    rc = np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1)
    if c.complex_ is not None:
        rc[sub] = c.complex_
    dt = 0.01 * r.normal(size=(n, 3))
    dr = 0.3 * r.normal(size=(n, 4)) + np.array([1.0, 0, 0, 0])
    if c.delta_r is not None:
        cyc = np.atleast_2d(np.asarray(c.delta_r, np.float64))
        dr[sub] = cyc[(np.arange(n) % G)[sub] % len(cyc)]
    return np.log(es), rc, dt, dr


@dataclass
class Batch:
    kind: str
    G: int
    loose: bool
    cases: list
    t: dict                                  # float32 / int64 torch tensors on the CPU: the launch's arguments and loss weights
    lo: float
    hi: float
    vrange: list = field(default_factory=list)   # per case: (first vertex, end), (first face, end)
    frange: list = field(default_factory=list)

    def grange(self, i):
        return self.frange[i][0] * self.G, self.frange[i][1] * self.G

    def names(self):
        return ["verts", "raw_scales", "raw_complex"] + (["delta_t", "delta_r"] if self.loose else [])

    def subject_gaussians(self, degenerate_only=True):
        """[N] bool: Gaussians of the subject faces of the (degenerate) cases."""
        m = np.concatenate([np.repeat(c.subject & (c.degenerate or not degenerate_only), self.G) for c in self.cases])
        return torch.from_numpy(m)


def _assemble(kind, G, loose, cases, params):
    vs, fs, vr, fr = [], [], [], []
    nv = nf = 0
    for c in cases:
        vs.append(c.verts); fs.append(c.faces + nv)
        vr.append((nv, nv + len(c.verts))); fr.append((nf, nf + len(c.faces)))
        nv += len(c.verts); nf += len(c.faces)
    cat = lambda k: torch.from_numpy(_f32(np.concatenate([p[k] for p in params])))
    t = dict(verts=torch.from_numpy(np.concatenate(vs)), faces=torch.from_numpy(np.concatenate(fs)).long(),
             bary=torch.from_numpy(bary_coords(G)), raw_scales=cat(0), raw_complex=cat(1),
             delta_t=cat(2) if loose else None, delta_r=cat(3) if loose else None)
    N = nf * G
    g = torch.Generator().manual_seed(zlib.crc32(f"{kind}/{G}/{int(loose)}".encode()))
    t.update(wp=torch.randn(N, 3, generator=g), ws=torch.randn(N, 3, generator=g), wq=torch.randn(N, 3, generator=g),
             W3=torch.randn(3, 3, generator=g), wq4=torch.randn(N, 4, generator=g))
    clamped = kind == "clamped"
    return Batch(kind, G, loose, list(cases), t, LO if clamped else None, HI if clamped else None, vr, fr)


@functools.lru_cache(maxsize=None)
def make_batch(kind, G, loose):
    cases = batch_cases(kind, loose)
    params = [_case_params(c, G, loose) for c in cases]
    b = _assemble(kind, G, loose, cases, params)
    if kind == "frames":
        # the oracle is smooth only away from a change of candidate: redraw the in-plane rotation (and delta_r) of every
        # Gaussian whose two largest q_abs are closer than 1e-3 in float64
        r = np.random.default_rng(G + 100 * int(loose))
        for _ in range(50):
            gap = q_abs_gap(b)
            bad = np.nonzero(gap.numpy() <= 2e-3)[0]
            if len(bad) == 0:
                break
            ang = r.uniform(0, 2 * np.pi, len(bad))
            b.t["raw_complex"][bad] = torch.from_numpy(_f32(np.stack([np.cos(ang), np.sin(ang)], -1)))
        else:
            raise AssertionError("frames: no smooth draw found")
    return b


def without_subjects(b):
    """The batch without the subject faces of its degenerate cases (vertices and every other face's parameters and weights
    stay): (batch, [N] bool mask of the Gaussians kept)."""
    keep_f = np.concatenate([~(c.subject & c.degenerate) for c in b.cases])
    keep_g = torch.from_numpy(np.repeat(keep_f, b.G))
    per_gaussian = ("raw_scales", "raw_complex", "delta_t", "delta_r", "wp", "ws", "wq", "wq4")
    t = {k: (v[keep_g] if k in per_gaussian and v is not None else v) for k, v in b.t.items()}
    t["faces"] = b.t["faces"][torch.from_numpy(keep_f)]
    return Batch(b.kind, b.G, b.loose, b.cases, t, b.lo, b.hi, b.vrange, None), keep_g


# ----------------------------------------------------------------------------------------------------------- running
def quat_R(q):
    """R(q) the way the rasterizer reads it: polynomial in q, no normalisation inside."""
    r, i, j, k = q.unbind(-1)
    return torch.stack((1 - 2 * (j * j + k * k), 2 * (i * j - k * r), 2 * (i * k + j * r), 2 * (i * j + k * r),
                        1 - 2 * (i * i + k * k), 2 * (j * k - i * r), 2 * (i * k - j * r), 2 * (j * k + i * r),
                        1 - 2 * (i * i + j * j)), -1).reshape(-1, 3, 3)


def loss_of(b, p, s, q, q_sign=None, mute=None):
    """The R(q) loss of tests/test_gpu_producers.py with random weights; with q_sign ([N], +-1) additionally
    sum(w q q_sign), a loss on the unit quaternion itself.  mute ([N] bool): those Gaussians get zero weight."""
    dev, dt = p.device, p.dtype
    w = {k: b.t[k].to(dev, dt) for k in ("wp", "ws", "wq", "W3", "wq4")}
    live = torch.ones(p.size(0), 1, device=dev, dtype=dt) if mute is None else (~mute).to(dev, dt)[:, None]
    loss = (p * w["wp"] * live).sum() + (s * w["ws"] * live).sum() + ((quat_R(q) @ w["W3"]) * (w["wq"] * live)[:, :, None]).sum()
    if q_sign is not None:
        loss = loss + (w["wq4"] * live * q * q_sign.to(dev, dt)[:, None]).sum()
    return loss


def run(fn, b, dev="cpu", dtype=torch.float32, q_sign=None, mute=None):
    """fn(verts, faces, bary, raw_scales, raw_complex, thickness, min, max, delta_t, delta_r) on the batch ->
    dict(points, scaling, quats, grads {name: tensor}), everything on the CPU."""
    a = {k: b.t[k].detach().clone().to(dev, dtype).requires_grad_(True) for k in b.names()}
    p, s, q = fn(a["verts"], b.t["faces"].to(dev), b.t["bary"].to(dev, dtype), a["raw_scales"], a["raw_complex"], THICKNESS, b.lo,
                 b.hi, a.get("delta_t"), a.get("delta_r"))
    loss_of(b, p, s, q, q_sign, mute).backward()
    return dict(points=p.detach().cpu(), scaling=s.detach().cpu(), quats=q.detach().cpu(),
                grads={k: a[k].grad.detach().cpu() for k in b.names()})


def run_f64(b, q_sign=None, mute=None):
    """The float64 reference.  Differentiated with respect to the gathered verts[faces], so that every face corner's own
    contribution to a vertex gradient is known: grads["verts"] is their sum, `corner_abs` [V] the per-vertex sum of the
    corners' largest absolute component -- what the order of the kernel's atomics and its LDS vertex table can move."""
    faces = b.t["faces"]
    F = faces.size(0)
    corners = b.t["verts"].detach().double()[faces].reshape(3 * F, 3).clone().requires_grad_(True)
    a = {k: b.t[k].detach().double().requires_grad_(True) for k in b.names() if k != "verts"}
    seen = {}
    m2q = po.matrix_to_quaternion

    def spy(m):
        seen["R"] = m.detach()
        return m2q(m)

    po.matrix_to_quaternion = spy
    try:
        p, s, q = po.mesh_bound_gaussians(corners, torch.arange(3 * F).reshape(F, 3), b.t["bary"].double(), a["raw_scales"],
                                          a["raw_complex"], THICKNESS, b.lo, b.hi, a.get("delta_t"), a.get("delta_r"))
    finally:
        po.matrix_to_quaternion = m2q
    loss_of(b, p, s, q, q_sign, mute).backward()
    V = b.t["verts"].size(0)
    cg = corners.grad.detach()
    gv = torch.zeros(V, 3, dtype=torch.float64).index_add_(0, faces.reshape(-1), cg)
    cabs = torch.zeros(V, dtype=torch.float64).index_add_(0, faces.reshape(-1), cg.abs().amax(-1))
    grads = {k: v.grad.detach() for k, v in a.items()}
    grads["verts"] = gv
    return dict(points=p.detach(), scaling=s.detach(), quats=q.detach(), grads=grads, corner_abs=cabs, R=seen["R"])


def oracle_R(b, dtype):
    """The matrices [N,3,3] the oracle hands to matrix_to_quaternion in `dtype`."""
    seen = {}
    m2q = po.matrix_to_quaternion

    def spy(m):
        seen["R"] = m.detach()
        return m2q(m)

    po.matrix_to_quaternion = spy
    try:
        with torch.no_grad():
            c = lambda k: None if b.t[k] is None else b.t[k].to(dtype)
            po.mesh_bound_gaussians(c("verts"), b.t["faces"], c("bary"), c("raw_scales"), c("raw_complex"), THICKNESS, b.lo, b.hi,
                                    c("delta_t"), c("delta_r"))
    finally:
        po.matrix_to_quaternion = m2q
    return seen["R"]


def q_abs_of(R):
    """The four q_abs of matrix_to_quaternion for matrices [N,3,3]."""
    d = torch.diagonal(R, dim1=-2, dim2=-1)
    sg = torch.tensor([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=R.dtype)
    return (1.0 + d @ sg.T).clamp(min=0).sqrt()


def q_abs_gap(b):
    """[N] largest minus second-largest q_abs, float64."""
    top = q_abs_of(run_f64(b)["R"]).topk(2, dim=-1).values
    return top[:, 0] - top[:, 1]


def masks(b, dtype):
    """Which side of every clamp the oracle takes in `dtype`: (scale passes both clamps [N,2], |n| > 1e-6 [F])."""
    e = torch.exp(b.t["raw_scales"].to(dtype))
    ok = torch.ones_like(e, dtype=torch.bool)
    if b.hi is not None:
        ok = (e <= b.hi) & (e.clamp(max=b.hi) >= b.lo)
    fv = b.t["verts"].to(dtype)[b.t["faces"]]
    n = torch.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=-1).norm(dim=-1)
    return ok, n > NORMAL_CLAMP


@functools.lru_cache(maxsize=None)
def reference(kind, G, loose):
    """(batch, float64 run, float32 run, e32) under the R(q) loss -- computed once, shared, never modified."""
    b = make_batch(kind, G, loose)
    r64, r32 = run_f64(b), run(po.mesh_bound_gaussians, b)
    return b, r64, r32, case_errors(b, r32, r64)


# ----------------------------------------------------------------------------------------------------------- errors
def norm_err(a, ref):
    """max|a - ref| / max|ref| over one case's rows; where the reference is all zero the result must be, too."""
    a, ref = a.double(), ref.double()
    if ref.numel() == 0:
        return 0.0
    top = float(ref.abs().max())
    d = float((a - ref).abs().max())
    if top == 0.0:
        return 0.0 if d == 0.0 else math.inf
    return d / top


def vertex_err(a, r64, lo=0, hi=None):
    """Per vertex: largest |a - b| component over the float64 sum of absolute per-corner contributions; -> the maximum."""
    d = (a.double() - r64["grads"]["verts"]).abs().amax(-1)[lo:hi]
    den = r64["corner_abs"][lo:hi]
    e = torch.where(den > 0, d / den.clamp(min=1e-300), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, math.inf)))
    return float(e.max()) if e.numel() else 0.0


def case_errors(b, got, r64):
    """{(case index, tensor name): normalised error}.  Tensors: "R" (rotation, through R(q)), "raw_complex", "delta_t", "delta_r"
    (per-Gaussian gradients over the case's largest |reference|), "verts" (vertex_err).  Degenerate cases are left out:
    run and autograd are both junk there, and differ."""
    out = {}
    Rg, Rr = quat_R(got["quats"].double()), quat_R(r64["quats"])
    for i, c in enumerate(b.cases):
        if c.degenerate:
            continue
        g0, g1 = b.grange(i)
        out[(i, "R")] = norm_err(Rg[g0:g1], Rr[g0:g1])
        for k in b.names():
            if k == "verts":
                out[(i, k)] = vertex_err(got["grads"][k], r64, *b.vrange[i])
            elif k != "raw_scales":
                out[(i, k)] = norm_err(got["grads"][k][g0:g1], r64["grads"][k][g0:g1])
    return out


def bound(e32, tensor):
    return max(EDGE_FACTORS[tensor] * e32, ERR_FLOOR)


def points_bound(b, r64=None):
    """4 * 2^-24 * sum_k |b_k v_k| + 2^-24 |delta_t| per component: the rounding of the three products and their sums."""
    fv = b.t["verts"].double()[b.t["faces"]]                                     # [F,3,3]
    s = (fv.abs()[:, None] * b.t["bary"].double()[None, :, :, None]).sum(-2).reshape(-1, 3)
    dt = b.t["delta_t"].double().abs() if b.loose else 0.0
    return 2.0 ** -24 * (4 * s + dt)


def check_points_and_scales(b, got, r64):
    """Points within points_bound, scales within the project's rtol = 2e-6 (__expf) with the clamps taken exactly; the
    gradient of raw_scales is (upstream * exp) behind the same mask: the same rtol, and zero exactly where the reference is."""
    dp = (got["points"].double() - r64["points"]).abs()
    assert bool((dp <= points_bound(b)).all()), f"points: {float((dp / points_bound(b)).max()):.3f} x the rounding bound"
    s, s64 = got["scaling"].double(), r64["scaling"]
    assert bool(((s - s64).abs() <= 2e-6 * s64.abs()).all()), f"scales: rtol {float(((s - s64).abs() / s64.abs()).max()):.3e}"
    if b.hi is not None:
        for v in (b.lo, b.hi):
            v32 = float(torch.tensor(v, dtype=torch.float32))
            assert bool(((s[:, 1:] == v32) == (s64[:, 1:] == v)).all()), "scales: clamp decisions differ"
    g, g64 = got["grads"]["raw_scales"].double(), r64["grads"]["raw_scales"]
    assert bool(((g == 0) == (g64 == 0)).all()), "raw_scales gradient: clamp mask differs"
    assert bool(((g - g64).abs() <= 2e-6 * g64.abs()).all()), \
        f"raw_scales gradient: rtol {float(((g - g64).abs() / g64.abs().clamp(min=1e-300)).max()):.3e}"


def all_finite(r):
    return all(bool(torch.isfinite(t).all()) for t in (r["points"], r["scaling"], r["quats"], *r["grads"].values()))


# ----------------------------------------------------------------------------------------------------------- the R0 rule
def r0_vertex_grads(fv, g, rule):
    """Vertex gradients [3,3] of g . R0(fv) by frame_backward's rule for R0 = normalize(n / max(|n|, 1e-6)), n = e1 x e2, in
    float64 numpy.  rule "single": one normalisation with eps 1e-6 (1e6 g below the clamp); rule "double": both."""
    def normalize_bwd(unit, ln, eps, gg):
        inv = 1.0 / max(ln, eps)
        return inv * (gg - np.dot(gg, unit) * unit) if ln > eps else inv * gg

    e1, e2 = fv[1] - fv[0], fv[2] - fv[0]
    n = np.cross(e1, e2)
    ln = np.linalg.norm(n)
    n0 = n / max(ln, 1e-6)
    R0 = n0 / max(np.linalg.norm(n0), 1e-12)
    if rule == "single" or ln > 1e-6:
        gn = normalize_bwd(R0, ln, 1e-6, g)
    else:
        gn = 1e6 * normalize_bwd(R0, ln * 1e6, 1e-12, g)
    ge1, ge2 = np.cross(e2, gn), np.cross(gn, e1)
    return np.stack([-(ge1 + ge2), ge1, ge2])
