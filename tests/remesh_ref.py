"""A numpy / plain-Python restatement of gaustar_amd.remesh (csrc/gsr_remesh.hip): the same rules, the same dtypes and the
same order of every floating-point operation, so the GPU result can be compared bit for bit.  Python floats are IEEE doubles
and +, -, *, / and sqrt round correctly on both sides; nothing here is fused.

    simplify(verts, faces, target, locked=None, attrs=())   the round-based parallel edge collapse -> Simplified
    greedy_simplify(verts, faces, target, locked=None)      a sequential heap-based decimator with the same quadrics, placement,
                                                            link and flip rules, ordered by the exact f64 cost: the quality
                                                            yardstick only, nothing on the GPU follows it
    smooth(verts, faces, steps, lambdas, weights, locked)   Laplacian (lambdas = (l, l)) / Taubin (lambdas = (l, mu)) sweeps
    select_round(...)                                       one round's selected edges, for the selection-rule test

and the small meshes both test files use (icosphere, bumpy, flat_grid, tetrahedron, octahedron, fin_mesh, degenerate_mesh).
"""
from __future__ import annotations

import heapq
import math
import struct
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

SENTINEL = 2 ** 63 - 1
DET_REL = 1e-10


# ------------------------------------------------------------------------------------------------ meshes
def icosphere(level: int) -> Tuple[np.ndarray, np.ndarray]:
    """The unit icosphere after `level` subdivisions: 20 * 4^level faces, outward winding.  verts f32, faces int32."""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    verts = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid = {}

        def midpoint(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[k] = len(verts) - 1
            return mid[k]

        nxt = []
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    return np.asarray(verts, np.float64).astype(np.float32), np.asarray(faces, np.int32)


def bump(d: np.ndarray) -> np.ndarray:
    """g(d) = 1 + 0.15 sin 3x sin 4y + 0.1 cos 5z for unit directions d [n,3] (f64)."""
    return 1.0 + 0.15 * np.sin(3.0 * d[:, 0]) * np.sin(4.0 * d[:, 1]) + 0.1 * np.cos(5.0 * d[:, 2])


def bumpy(level: int) -> Tuple[np.ndarray, np.ndarray]:
    """The icosphere scaled radially by g: the true surface is r = g(direction)."""
    v, f = icosphere(level)
    d = v.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * bump(d)[:, None]).astype(np.float32), f


def noisy_sphere(level: int, seed: int = 0, amp: float = 0.05) -> Tuple[np.ndarray, np.ndarray]:
    v, f = icosphere(level)
    r = 1.0 + amp * np.random.default_rng(seed).standard_normal(v.shape[0])
    return (v.astype(np.float64) * r[:, None]).astype(np.float32), f


def flat_grid(n: int = 9, z: float = 0.5) -> Tuple[np.ndarray, np.ndarray]:
    """n x n vertices at integer x, y in the plane z: 2 (n - 1)^2 faces with normal +z."""
    ys, xs = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    verts = np.stack([xs.reshape(-1), ys.reshape(-1), np.full(n * n, z)], 1).astype(np.float32)
    faces = []
    for j in range(n - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i, (j + 1) * n + i + 1
            faces += [(a, b, d), (a, d, c)]
    return verts, np.asarray(faces, np.int32)


def tetrahedron() -> Tuple[np.ndarray, np.ndarray]:
    v = np.asarray([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.float32)
    return v, np.asarray([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.int32)


def octahedron() -> Tuple[np.ndarray, np.ndarray]:
    v = np.asarray([(0, 0, 1), (1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (0, 0, -1)], np.float32)
    f = [(0, 1, 2), (0, 2, 3), (0, 3, 4), (0, 4, 1), (5, 2, 1), (5, 3, 2), (5, 4, 3), (5, 1, 4)]
    return v, np.asarray(f, np.int32)


def fin_mesh() -> Tuple[np.ndarray, np.ndarray, Tuple[int, int, int]]:
    """The level-1 icosphere with a third face on the edge of its first face: (verts, faces, (u, v, w)) with (u, v) the fin
    edge of three faces and w the fin's free corner."""
    v, f = icosphere(1)
    a, b = int(f[0, 0]), int(f[0, 1])
    tip = (1.5 * (v[a].astype(np.float64) + v[b].astype(np.float64))).astype(np.float32)
    w = v.shape[0]
    return np.concatenate([v, tip[None]]), np.concatenate([f, np.asarray([(b, a, w)], np.int32)]), (a, b, w)


def split_edge(verts: np.ndarray, faces: np.ndarray, p: int, q: int, pos: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Edge (p, q) split by a new vertex at `pos`: each of its faces becomes two."""
    m = verts.shape[0]
    out = []
    for c in faces.tolist():
        if p in c and q in c:
            i = c.index(p)
            c = c[i:] + c[:i]                     # (p, x, y)
            if c[1] == q:                         # (p, q, r) -> (p, m, r), (m, q, r)
                out += [(p, m, c[2]), (m, q, c[2])]
            else:                                 # (p, r, q) -> (p, r, m), (m, r, q)
                out += [(p, c[1], m), (m, c[1], q)]
        else:
            out.append(tuple(c))
    return np.concatenate([verts, np.asarray(pos, np.float32)[None]]), np.asarray(out, np.int32)


def degenerate_mesh() -> Tuple[np.ndarray, np.ndarray]:
    """The level-2 icosphere with one edge split by a vertex AT one of its ends (two faces of exactly zero area) and another
    split very close to one end (two slivers).  Closed and manifold by its indices."""
    v, f = icosphere(2)
    p, q = int(f[0, 0]), int(f[0, 1])
    v, f = split_edge(v, f, p, q, v[p])
    p2, q2 = int(f[100, 0]), int(f[100, 1])
    near = v[p2].astype(np.float64) + 1e-5 * (v[q2].astype(np.float64) - v[p2].astype(np.float64))
    return split_edge(v, f, p2, q2, near.astype(np.float32))


# ------------------------------------------------------------------------------------------------ geometry (Python floats)
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def face_quadric(x0, x1, x2) -> List[float]:
    n = _cross(_sub(x1, x0), _sub(x2, x0))
    s = _dot(n, n)
    length = math.sqrt(s) if s >= 0.0 else float("nan")
    p = [0.0, 0.0, 0.0, 0.0]
    A = 0.0
    if length > 0.0:
        p[0], p[1], p[2] = n[0] / length, n[1] / length, n[2] / length
        p[3] = -((p[0] * x0[0] + p[1] * x0[1]) + p[2] * x0[2])
        A = length * 0.5
    return [A * (p[i] * p[j]) for i in range(4) for j in range(i, 4)]


def quadric_cost(q, p) -> float:
    r0 = ((q[0] * p[0] + q[1] * p[1]) + q[2] * p[2]) + q[3]
    r1 = ((q[1] * p[0] + q[4] * p[1]) + q[5] * p[2]) + q[6]
    r2 = ((q[2] * p[0] + q[5] * p[1]) + q[7] * p[2]) + q[8]
    r3 = ((q[3] * p[0] + q[6] * p[1]) + q[8] * p[2]) + q[9]
    c = ((p[0] * r0 + p[1] * r1) + p[2] * r2) + r3
    return 0.0 if c < 0.0 else c


def place(q, pu, pv):
    """(position, cost) of the merged vertex under Q = q."""
    c00, c01, c02 = q[4] * q[7] - q[5] * q[5], q[1] * q[7] - q[5] * q[2], q[1] * q[5] - q[4] * q[2]
    det = (q[0] * c00 - q[1] * c01) + q[2] * c02
    s = 0.0
    for t in (0, 1, 2, 4, 5, 7):
        a = abs(q[t])
        if a > s:
            s = a
    if abs(det) > DET_REL * ((s * s) * s):
        b0, b1, b2 = -q[3], -q[6], -q[8]
        m0, m1, m2 = b1 * q[7] - q[5] * b2, b1 * q[5] - q[4] * b2, q[1] * b2 - b1 * q[2]
        dx = (b0 * c00 - q[1] * m0) + q[2] * m1
        dy = (q[0] * m0 - b0 * c01) + q[2] * m2
        dz = (b0 * c02 - q[0] * m1) - q[1] * m2
        best = (dx / det, dy / det, dz / det)
        return best, quadric_cost(q, best)
    mid = (0.5 * (pu[0] + pv[0]), 0.5 * (pu[1] + pv[1]), 0.5 * (pu[2] + pv[2]))
    cost, best = quadric_cost(q, pu), pu
    cv, cm = quadric_cost(q, pv), quadric_cost(q, mid)
    if cv < cost:
        cost, best = cv, pv
    if cm < cost:
        cost, best = cm, mid
    return best, cost


def f32_bits(x: float) -> Optional[int]:
    """The bits of x rounded to f32, None where that is not finite."""
    try:
        bits = struct.unpack("<I", struct.pack("<f", x))[0]
    except OverflowError:
        return None
    return None if (bits & 0x7f800000) == 0x7f800000 else bits


def keeps_side(P, c, u, v, x) -> bool:
    p = [P[c[0]], P[c[1]], P[c[2]]]
    y = [x if (c[k] == u or c[k] == v) else p[k] for k in range(3)]
    nb = _cross(_sub(p[1], p[0]), _sub(p[2], p[0]))
    na = _cross(_sub(y[1], y[0]), _sub(y[2], y[0]))
    d = _dot(nb, na)
    if d < 0.0:
        return False
    if d == 0.0 and (nb[0] != 0.0 or nb[1] != 0.0 or nb[2] != 0.0):
        return False
    return True


def candidate(u: int, v: int, faces, vf, P, Q):
    """None where edge (u, v) -- manifold, both ends free -- is no candidate, else (f32 cost bits, f64 cost, position)."""
    opp = []
    for f in vf[u]:
        c = faces[f]
        if v in c:
            opp.append(c[0] if c[0] != u and c[0] != v else c[1] if c[1] != u and c[1] != v else c[2])
    if len(opp) != 2:
        return None
    a, b = opp
    if a == b or a in (u, v) or b in (u, v):
        return None
    near_v = set()
    for g in vf[v]:
        near_v.update(faces[g])
    uab = False
    for f in vf[u]:
        c = faces[f]
        if v in c:
            continue
        uab = uab or (a in c and b in c)
        for w in c:
            if w != u and w != a and w != b and w in near_v:
                return None
    vab = any(u not in faces[g] and a in faces[g] and b in faces[g] for g in vf[v])
    if uab and vab:
        return None
    q = [Q[u][t] + Q[v][t] for t in range(10)]
    x, cost = place(q, P[u], P[v])
    bits = f32_bits(cost)
    if bits is None:
        return None
    for w, other in ((u, v), (v, u)):
        for f in vf[w]:
            c = faces[f]
            if other in c:
                continue
            if not keeps_side(P, c, u, v, x):
                return None
    return bits & 0x7fffffff, cost, x


# ------------------------------------------------------------------------------------------------ the working state
class _State:
    def __init__(self, verts: np.ndarray, faces: np.ndarray, locked, attrs):
        verts = np.asarray(verts)
        faces = np.asarray(faces)
        assert verts.dtype == np.float32 and verts.ndim == 2 and verts.shape[1] == 3
        self.V, self.F = int(verts.shape[0]), int(faces.shape[0])
        if self.F and (faces.min() < 0 or faces.max() >= self.V):
            raise ValueError("a vertex index, or another index into the mesh, lies outside its array")
        self.P = [tuple(p) for p in verts.astype(np.float64).tolist()]
        self.faces = [list(c) for c in faces.astype(np.int64).tolist()]
        self.live = [True] * self.F
        self.locked = np.zeros(self.V, bool) if locked is None else np.asarray(locked).astype(bool).copy()
        self.attrs = [np.array(a, np.float32, copy=True) for a in attrs]
        K = [face_quadric(self.P[c[0]], self.P[c[1]], self.P[c[2]]) for c in self.faces]
        self.Q = []
        for lst in self.vertex_faces():
            q = [0.0] * 10
            for f in lst:
                k = K[f]
                for t in range(10):
                    q[t] += k[t]
            self.Q.append(q)

    def vertex_faces(self) -> List[List[int]]:
        """Per vertex its live incidences' faces in ascending 3 face + corner."""
        vf = [[] for _ in range(self.V)]
        for f in range(self.F):
            if self.live[f]:
                for w in self.faces[f]:
                    vf[w].append(f)
        return vf

    def edges(self):
        """(edges [(u, v)] in ascending key order, manifold [bool], fixed [V] bool)."""
        runs = {}
        for f in range(self.F):
            if self.live[f]:
                c = self.faces[f]
                for k in range(3):
                    a, b = c[k], c[(k + 1) % 3]
                    runs.setdefault((min(a, b), max(a, b)), []).append(f)
        keys = sorted(runs)
        fixed = self.locked.copy()
        manifold = []
        for u, v in keys:
            r = runs[(u, v)]
            two = len(r) == 2 and r[0] != r[1] and u != v
            manifold.append(two)
            if not two:
                fixed[u] = fixed[v] = True
        return keys, manifold, fixed

    def collapse(self, u: int, v: int, x, vf) -> None:
        self.Q[u] = [self.Q[u][t] + self.Q[v][t] for t in range(10)]
        self.P[u] = tuple(x)
        for a in self.attrs:
            a[u] = (a[u] + a[v]) * np.float32(0.5)
        for f in vf[v]:
            c = self.faces[f]
            if u in c:
                self.live[f] = False
            else:
                self.faces[f] = [u if w == v else w for w in c]

    def n_live(self) -> int:
        return sum(self.live)

    def emit(self, n_rounds: int, stalled: bool) -> "Simplified":
        origin = np.asarray([f for f in range(self.F) if self.live[f]], np.int32)
        fs = np.asarray([self.faces[f] for f in origin], np.int64).reshape(-1, 3)
        used = np.zeros(self.V, bool)
        used[fs.reshape(-1)] = True
        new = np.cumsum(used) - 1
        P = np.asarray(self.P, np.float64).reshape(-1, 3)
        return Simplified(verts=P[used].astype(np.float32), faces=new[fs].astype(np.int32), face_origin=origin,
                          attrs=tuple(a[used] for a in self.attrs), n_rounds=n_rounds, stalled=stalled)


@dataclass
class Simplified:
    verts: np.ndarray
    faces: np.ndarray
    face_origin: np.ndarray
    attrs: Tuple[np.ndarray, ...]
    n_rounds: int
    stalled: bool


def _identity(verts, faces, attrs) -> Simplified:
    return Simplified(np.array(verts, np.float32), np.array(faces, np.int32), np.arange(len(faces), dtype=np.int32),
                      tuple(np.array(a, np.float32) for a in attrs), 0, False)


# ------------------------------------------------------------------------------------------------ the parallel rounds
def select_round(state: _State):
    """One round up to the independent set: (edges, selected [(key, edge id)] ascending, placements {edge id: x}, vf)."""
    edges, manifold, fixed = state.edges()
    vf = state.vertex_faces()
    key = {}
    where = {}
    for e, (u, v) in enumerate(edges):
        if manifold[e] and not fixed[u] and not fixed[v]:
            c = candidate(u, v, state.faces, vf, state.P, state.Q)
            if c is not None:
                key[e] = (c[0] << 32) | e
                where[e] = c[2]
    m1 = {}
    for e, k in key.items():
        for w in edges[e]:
            m1[w] = min(m1.get(w, SENTINEL), k)
    m2 = {}
    for u, v in edges:                       # every edge of the mesh, candidate or not
        m = min(m1.get(u, SENTINEL), m1.get(v, SENTINEL))
        m2[u] = min(m2.get(u, SENTINEL), m)
        m2[v] = min(m2.get(v, SENTINEL), m)
    selected = sorted((k, e) for e, k in key.items() if m2[edges[e][0]] == k and m2[edges[e][1]] == k)
    return edges, selected, where, vf


def simplify(verts, faces, target: int, locked=None, attrs: Sequence[np.ndarray] = ()) -> Simplified:
    target = int(target)
    if target < 0:
        raise ValueError("target_faces must not be negative")
    if target >= len(faces):
        return _identity(verts, faces, attrs)
    st = _State(verts, faces, locked, attrs)
    live, rounds, stalled = st.F, 0, False
    while live > target:
        edges, selected, where, vf = select_round(st)
        if not selected:
            stalled = True
            break
        n = min(len(selected), (live - target + 1) // 2)
        for _k, e in selected[:n]:
            st.collapse(edges[e][0], edges[e][1], where[e], vf)
        live -= 2 * n
        rounds += 1
    return st.emit(rounds, stalled)


# ------------------------------------------------------------------------------------------------ the sequential yardstick
def greedy_simplify(verts, faces, target: int, locked=None) -> Simplified:
    """Always the cheapest legal collapse by the exact f64 cost (edge key on ties), one at a time, with a heap and lazy
    invalidation: after a collapse the edges at the survivor and at its neighbours are evaluated afresh."""
    target = int(target)
    if target >= len(faces):
        return _identity(verts, faces, ())
    st = _State(verts, faces, locked, ())
    _edges, _manifold, fixed = st.edges()        # (interior collapses leave every other edge's multiplicity alone)
    vf = st.vertex_faces()
    stamp = [0] * st.V
    heap = []

    def push_edges_at(w, seen):
        for f in vf[w]:
            for z in st.faces[f]:
                u, v = min(w, z), max(w, z)
                if z == w or (u, v) in seen or fixed[u] or fixed[v]:
                    continue
                seen.add((u, v))
                c = candidate(u, v, st.faces, vf, st.P, st.Q)
                if c is not None:
                    heapq.heappush(heap, (c[1], u, v, stamp[u], stamp[v], c[2]))

    seen = set()
    for w in range(st.V):
        push_edges_at(w, seen)
    live, steps = st.F, 0
    while live > target and heap:
        _cost, u, v, su, sv, x = heapq.heappop(heap)
        if stamp[u] != su or stamp[v] != sv:
            continue
        st.collapse(u, v, x, vf)
        merged = [f for f in vf[v] if st.live[f]]
        vf[u] = sorted(set(f for f in vf[u] if st.live[f]) | set(merged))
        vf[v] = []
        ring = {u}
        for f in vf[u]:
            ring.update(st.faces[f])
        for w in ring:
            vf[w] = [f for f in vf[w] if st.live[f]]
            stamp[w] += 1
        stamp[v] += 1
        seen = set()
        for w in ring:
            push_edges_at(w, seen)
        live -= 2
        steps += 1
    return st.emit(steps, live > target)


# ------------------------------------------------------------------------------------------------ smoothing
def vertex_neighbours(faces: np.ndarray, V: int) -> List[np.ndarray]:
    """Per vertex its neighbours along the unique edges, ascending (MeshTopology.vertex_neighbours)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [1, 2]], f[:, [2, 0]], f[:, [0, 1]]])
    e = np.unique(np.sort(e, axis=1), axis=0) if len(e) else e
    nb = [[] for _ in range(V)]
    for a, b in e.tolist():
        nb[a].append(b)
        nb[b].append(a)
    return [np.asarray(sorted(x), np.int64) for x in nb]


def smooth(verts, faces, steps: int, lambdas: Tuple[float, float], weights: str = "inverse_distance", locked=None) -> np.ndarray:
    """`steps` sweeps, sweep s with lambdas[s & 1]; f64 inside, f32 in and out."""
    verts = np.asarray(verts)
    assert verts.dtype == np.float32
    V = verts.shape[0]
    nb = vertex_neighbours(faces, V)
    deg = np.asarray([len(x) for x in nb])
    width = int(deg.max()) if V else 0
    table = np.zeros((V, max(width, 1)), np.int64)
    for i, x in enumerate(nb):
        table[i, :len(x)] = x
    moving = deg > 0
    if locked is not None:
        moving &= ~np.asarray(locked).astype(bool)
    P = verts.astype(np.float64)
    for s in range(int(steps)):
        lam = float(lambdas[s & 1])
        acc = np.zeros((V, 3))
        sw = np.zeros(V)
        for j in range(width):                   # slot by slot: every vertex adds its neighbours in ascending order
            on = deg > j
            q = P[table[:, j]]
            if weights == "uniform":
                w = np.ones(V)
            else:
                d = P - q
                w = 1.0 / (np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + 1e-12)
            acc = np.where(on[:, None], acc + w[:, None] * q, acc)
            sw = np.where(on, sw + w, sw)
        with np.errstate(invalid="ignore", divide="ignore"):
            new = P + lam * (acc / sw[:, None] - P)
        P = np.where(moving[:, None], new, P)
    return P.astype(np.float32)
