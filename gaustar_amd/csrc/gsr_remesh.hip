// gsr_remesh.hip -- quadric mesh decimation and Laplacian / Taubin smoothing: what extract_mesh_fusion's `simplify_face_num` and
// `smooth` do with Open3D (gaustar_trainers/refined_mesh.py:451-458) and what makes an init_mesh_100k.obj (pyfqmr's
// simplify_mesh, gaustar_tools/cmr_convert.py:262-266), as this project's own statement of Garland-Heckbert decimation: a
// round-based parallel edge collapse (gaustar_amd.remesh has the rules in full).  One round, over device tensors:
//   keys                remesh_key_kernel          per live face three edge keys (min << 32 | max), three corner keys
//                                                  (vertex 3F + 3 face + corner) and the vertices' degrees (integer adds)
//                       (torch.sort of both key arrays, torch.cumsum of the degrees: the vertex -> face lists)
//   edges               remesh_head_kernel         1 at the first sorted key of every run
//                       (torch.cumsum: an edge's id is its rank among the unique keys)
//                       remesh_edge_kernel         per edge its two vertices and whether exactly two face-edges of two different
//                                                  faces have it; the ends of every other edge are fixed
//   candidates          remesh_candidate_kernel    link condition, placement (Cramer's rule, or the cheapest of the two ends and
//                                                  the midpoint), cost, flip test; key = f32(cost) bits << 32 | edge id
//   independent set     remesh_min1 / min2 / pick_kernel   three passes of 64-bit integer atomicMin
//                       (torch.sort of the selected keys: the cap)
//   apply               remesh_apply_kernel, remesh_attr_kernel
// and once: remesh_widen_kernel, remesh_face_quadric_kernel, remesh_vertex_quadric_kernel.  Smoothing is remesh_smooth_kernel,
// ping-pong over two f64 buffers.  Geometry is f64 without contraction, every sum in one stated order; no float atomics: the
// same inputs give the same bits, the bits tests/remesh_ref.py gives.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_surface.h"

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int RM_BLOCK = MESH_BLOCK;
constexpr long long RM_SENTINEL = 0x7fffffffffffffffll;   // above every key
constexpr double RM_DET_REL = 1e-10;                       // Cramer's rule iff |det| > RM_DET_REL s^3, s = the largest |entry| of the 3x3

// the vertex -> face lists of one round: vertex v's live incidences are corners[off[v] .. off[v + 1]) in ascending 3 face + corner
struct VertexFaces {
    const int* off;
    const long long* corners;
    long long n3;   // 3 F
    __device__ __forceinline__ int begin(int v) const { const int b = off[v]; return b < 0 ? 0 : b; }
    __device__ __forceinline__ int end(int v) const { const int e = off[v + 1]; return (long long)e > n3 ? (int)n3 : e; }
    // the face of entry i of vertex v's list, -1 for an entry that is none of v's
    __device__ __forceinline__ int face(int v, int i) const
    {
        const long long c = corners[i] - (long long)v * n3;
        return c >= 0 && c < n3 ? (int)(c / 3) : -1;
    }
};

// ---------------------------------------------------------------------------------------------------- setup
__global__ void __launch_bounds__(RM_BLOCK) remesh_widen_kernel(long long n, const float* __restrict__ in, double* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * RM_BLOCK + threadIdx.x;
    if (i < n) out[i] = (double)in[i];
}

__global__ void __launch_bounds__(RM_BLOCK) remesh_narrow_kernel(long long n, const double* __restrict__ in, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * RM_BLOCK + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}

// K_f = A p p^T, p = (n / |n|, -(n / |n|) . x0), n = (x1 - x0) x (x2 - x0), A = |n| / 2: the 10 values aa ab ac ad bb bc bd cc cd dd.
// A face with an index outside [0, V) is not live (err bit 0); one with |n| == 0 (or NaN) contributes zeros.
__global__ void __launch_bounds__(RM_BLOCK) remesh_face_quadric_kernel(int F, int V, const int* __restrict__ faces, const double* __restrict__ pos,
                                                                       int* __restrict__ live, double* __restrict__ K, int* __restrict__ err)
{
    const int f = blockIdx.x * RM_BLOCK + threadIdx.x;
    if (f >= F) return;
    double* k = K + 10 * (size_t)f;
    int v[3];
    const bool ok = mesh_face(faces, f, V, v);
    live[f] = ok;
    double p[4] = {0.0, 0.0, 0.0, 0.0}, A = 0.0;
    if (!ok) {
        atomicOr(err, MESH_ERR_INDEX);
    } else {
        const D3 x0 = load3(pos, (size_t)v[0]);
        const D3 n = cross3(sub3(load3(pos, (size_t)v[1]), x0), sub3(load3(pos, (size_t)v[2]), x0));
        const double len = sqrt(dot3(n, n));
        if (len > 0.0) {
            p[0] = n.x / len; p[1] = n.y / len; p[2] = n.z / len;
            p[3] = -((p[0] * x0.x + p[1] * x0.y) + p[2] * x0.z);
            A = len * 0.5;
        }
    }
    int t = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j) k[t++] = A * (p[i] * p[j]);
}

// Q_v = the sum of K_f over v's incidences in ascending face order, from 0
__global__ void __launch_bounds__(RM_BLOCK) remesh_vertex_quadric_kernel(int V, VertexFaces vf, const double* __restrict__ K, double* __restrict__ Q)
{
    const int v = blockIdx.x * RM_BLOCK + threadIdx.x;
    if (v >= V) return;
    double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = vf.begin(v); i < vf.end(v); ++i) {
        const int f = vf.face(v, i);
        if (f < 0) continue;
        const double* k = K + 10 * (size_t)f;
        for (int t = 0; t < 10; ++t) q[t] += k[t];
    }
    for (int t = 0; t < 10; ++t) Q[10 * (size_t)v + t] = q[t];
}

// ---------------------------------------------------------------------------------------------------- one round: keys and edges
__global__ void __launch_bounds__(RM_BLOCK) remesh_key_kernel(int F, int V, const int* __restrict__ faces, const int* __restrict__ live,
                                                              long long* __restrict__ ekeys, long long* __restrict__ ckeys, int* __restrict__ degree)
{
    const int f = blockIdx.x * RM_BLOCK + threadIdx.x;
    if (f >= F) return;
    int v[3];
    const bool on = live[f] != 0 && mesh_face(faces, f, V, v);
    long long* ek = ekeys + 3 * (size_t)f;
    long long* ck = ckeys + 3 * (size_t)f;
    const long long n3 = 3 * (long long)F;
    for (int k = 0; k < 3; ++k) {
        ek[k] = on ? edge_key(v[k], v[(k + 1) % 3]) : RM_SENTINEL;
        ck[k] = on ? (long long)v[k] * n3 + (3 * (long long)f + k) : RM_SENTINEL;
        if (on) atomicAdd(degree + v[k], 1);
    }
}

__global__ void __launch_bounds__(RM_BLOCK) remesh_head_kernel(int n, const long long* __restrict__ skeys, int* __restrict__ head)
{
    const int i = blockIdx.x * RM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long k = skeys[i];
    head[i] = k != RM_SENTINEL && (i == 0 || skeys[i - 1] != k);
}

// per unique edge (id = head_scan - 1 at the first key of its run): its vertices and manifold = exactly two face-edges of two
// different faces have it.  The ends of an edge that is not manifold are fixed (fixed [V] holds the caller's locked mask before).
__global__ void __launch_bounds__(RM_BLOCK) remesh_edge_kernel(int n, int V, const long long* __restrict__ skeys, const long long* __restrict__ order,
                                                               const int* __restrict__ head_scan, int* __restrict__ euv,
                                                               unsigned char* __restrict__ manifold, unsigned char* __restrict__ fixed)
{
    const int i = blockIdx.x * RM_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long k = skeys[i];
    if (k == RM_SENTINEL || (i > 0 && skeys[i - 1] == k)) return;
    const int e = head_scan[i] - 1;
    if (e < 0 || e >= n) return;
    int run = 1;
    while (run < 3 && i + run < n && skeys[i + run] == k) ++run;
    const int u = (int)(k >> 32), v = (int)(k & 0xffffffffll);
    const bool two = run == 2 && order[i] / 3 != order[i + 1] / 3 && u != v;
    euv[2 * (size_t)e] = u;
    euv[2 * (size_t)e + 1] = v;
    manifold[e] = two;
    if (!two) {
        if ((unsigned)u < (unsigned)V) fixed[u] = 1;
        if ((unsigned)v < (unsigned)V) fixed[v] = 1;
    }
}

// ---------------------------------------------------------------------------------------------------- candidates
struct Quadric { double q[10]; };   // aa ab ac ad bb bc bd cc cd dd

// max(x^T Q x, 0) with x = (p, 1): the four rows first, each ((a x + b y) + c z) + d, then ((x r0 + y r1) + z r2) + r3
__device__ __forceinline__ double quadric_cost(const Quadric& Q, D3 p)
{
    const double* q = Q.q;
    const double r0 = ((q[0] * p.x + q[1] * p.y) + q[2] * p.z) + q[3];
    const double r1 = ((q[1] * p.x + q[4] * p.y) + q[5] * p.z) + q[6];
    const double r2 = ((q[2] * p.x + q[5] * p.y) + q[7] * p.z) + q[8];
    const double r3 = ((q[3] * p.x + q[6] * p.y) + q[8] * p.z) + q[9];
    const double c = ((p.x * r0 + p.y * r1) + p.z * r2) + r3;
    return c < 0.0 ? 0.0 : c;      // (NaN stays NaN: its f32 is not finite, the edge no candidate)
}

__device__ __forceinline__ double abs_max(double a, double b) { const double x = fabs(b); return x > a ? x : a; }

// the position of the merged vertex and its cost
__device__ __forceinline__ double place(const Quadric& Q, D3 pu, D3 pv, D3& best)
{
    const double* q = Q.q;
    const double c00 = q[4] * q[7] - q[5] * q[5], c01 = q[1] * q[7] - q[5] * q[2], c02 = q[1] * q[5] - q[4] * q[2];
    const double det = (q[0] * c00 - q[1] * c01) + q[2] * c02;
    double s = abs_max(0.0, q[0]);
    s = abs_max(s, q[1]); s = abs_max(s, q[2]); s = abs_max(s, q[4]); s = abs_max(s, q[5]); s = abs_max(s, q[7]);
    if (fabs(det) > RM_DET_REL * ((s * s) * s)) {
        const double b0 = -q[3], b1 = -q[6], b2 = -q[8];
        const double m0 = b1 * q[7] - q[5] * b2, m1 = b1 * q[5] - q[4] * b2, m2 = q[1] * b2 - b1 * q[2];
        const double dx = (b0 * c00 - q[1] * m0) + q[2] * m1;
        const double dy = (q[0] * m0 - b0 * c01) + q[2] * m2;
        const double dz = (b0 * c02 - q[0] * m1) - q[1] * m2;
        best = {dx / det, dy / det, dz / det};
        return quadric_cost(Q, best);
    }
    const D3 mid = {0.5 * (pu.x + pv.x), 0.5 * (pu.y + pv.y), 0.5 * (pu.z + pv.z)};
    double cost = quadric_cost(Q, pu);
    best = pu;
    const double cv = quadric_cost(Q, pv), cm = quadric_cost(Q, mid);
    if (cv < cost) { cost = cv; best = pv; }
    if (cm < cost) { cost = cm; best = mid; }
    return cost;
}

__device__ __forceinline__ bool has(const int (&c)[3], int w) { return c[0] == w || c[1] == w || c[2] == w; }

// false where moving u and v to x turns face c over (n_before . n_after < 0) or flattens it (== 0 with n_before != 0)
__device__ __forceinline__ bool keeps_side(const double* __restrict__ pos, const int (&c)[3], int u, int v, D3 x)
{
    D3 p[3], y[3];
    for (int k = 0; k < 3; ++k) {
        p[k] = load3(pos, (size_t)c[k]);
        y[k] = (c[k] == u || c[k] == v) ? x : p[k];
    }
    const D3 nb = cross3(sub3(p[1], p[0]), sub3(p[2], p[0])), na = cross3(sub3(y[1], y[0]), sub3(y[2], y[0]));
    const double d = dot3(nb, na);
    if (d < 0.0) return false;
    if (d == 0.0 && (nb.x != 0.0 || nb.y != 0.0 || nb.z != 0.0)) return false;
    return true;
}

__device__ long long candidate_key(int e, int u, int v, int V, const VertexFaces& vf, const int* __restrict__ faces,
                                   const double* __restrict__ pos, const double* __restrict__ Qv, double* __restrict__ placement)
{
    // the edge's two faces and their opposite corners
    int opp[2] = {-1, -1}, on_edge = 0;
    for (int i = vf.begin(u); i < vf.end(u); ++i) {
        const int f = vf.face(u, i);
        int c[3];
        if (f < 0 || !mesh_face(faces, f, V, c)) return RM_SENTINEL;
        if (!has(c, v)) continue;
        const int w = c[0] != u && c[0] != v ? c[0] : c[1] != u && c[1] != v ? c[1] : c[2];
        if (on_edge < 2) opp[on_edge] = w;
        ++on_edge;
    }
    for (int j = vf.begin(v); j < vf.end(v); ++j) {      // (every entry of both lists is a face of the mesh from here on)
        const int g = vf.face(v, j);
        int d[3];
        if (g < 0 || !mesh_face(faces, g, V, d)) return RM_SENTINEL;
    }
    const int a = opp[0], b = opp[1];
    if (on_edge != 2 || a == b || a == u || a == v || b == u || b == v) return RM_SENTINEL;
    // link condition: the vertices adjacent to both ends are a and b only, and no face (u, a, b) faces a face (v, a, b)
    bool uab = false, vab = false;
    for (int i = vf.begin(u); i < vf.end(u); ++i) {
        int c[3];
        mesh_face(faces, vf.face(u, i), V, c);
        if (has(c, v)) continue;
        uab = uab || (has(c, a) && has(c, b));
        for (int k = 0; k < 3; ++k) {
            const int w = c[k];
            if (w == u || w == a || w == b) continue;
            for (int j = vf.begin(v); j < vf.end(v); ++j) {
                int d[3];
                mesh_face(faces, vf.face(v, j), V, d);
                if (has(d, w)) return RM_SENTINEL;
            }
        }
    }
    for (int j = vf.begin(v); j < vf.end(v); ++j) {
        int d[3];
        mesh_face(faces, vf.face(v, j), V, d);
        if (!has(d, u)) vab = vab || (has(d, a) && has(d, b));
    }
    if (uab && vab) return RM_SENTINEL;
    // placement and cost
    Quadric Q;
    for (int t = 0; t < 10; ++t) Q.q[t] = Qv[10 * (size_t)u + t] + Qv[10 * (size_t)v + t];
    D3 x;
    const double cost = place(Q, load3(pos, (size_t)u), load3(pos, (size_t)v), x);
    const unsigned bits = __float_as_uint((float)cost);
    if ((bits & 0x7f800000u) == 0x7f800000u) return RM_SENTINEL;
    // flip test over the other faces of u, then of v
    for (int side = 0; side < 2; ++side) {
        const int w = side ? v : u, other = side ? u : v;
        for (int i = vf.begin(w); i < vf.end(w); ++i) {
            int c[3];
            mesh_face(faces, vf.face(w, i), V, c);
            if (has(c, other)) continue;
            if (!keeps_side(pos, c, u, v, x)) return RM_SENTINEL;
        }
    }
    placement[3 * (size_t)e] = x.x;
    placement[3 * (size_t)e + 1] = x.y;
    placement[3 * (size_t)e + 2] = x.z;
    return ((long long)(bits & 0x7fffffffu) << 32) | (long long)(unsigned)e;
}

__global__ void __launch_bounds__(RM_BLOCK) remesh_candidate_kernel(int cap, const int* __restrict__ n_edges, int V, VertexFaces vf,
                                                                    const int* __restrict__ euv, const unsigned char* __restrict__ manifold,
                                                                    const unsigned char* __restrict__ fixed, const int* __restrict__ faces,
                                                                    const double* __restrict__ pos, const double* __restrict__ Q,
                                                                    long long* __restrict__ key, double* __restrict__ placement)
{
    const int e = blockIdx.x * RM_BLOCK + threadIdx.x;
    if (e >= cap) return;
    long long k = RM_SENTINEL;
    if (e < *n_edges && manifold[e]) {
        const int u = euv[2 * (size_t)e], v = euv[2 * (size_t)e + 1];
        if ((unsigned)u < (unsigned)V && (unsigned)v < (unsigned)V && u < v && !fixed[u] && !fixed[v])
            k = candidate_key(e, u, v, V, vf, faces, pos, Q, placement);
    }
    key[e] = k;
}

// ---------------------------------------------------------------------------------------------------- independent set
__global__ void __launch_bounds__(RM_BLOCK) remesh_fill_kernel(int n, long long* __restrict__ a, long long* __restrict__ b)
{
    const int i = blockIdx.x * RM_BLOCK + threadIdx.x;
    if (i >= n) return;
    a[i] = RM_SENTINEL;
    b[i] = RM_SENTINEL;
}

__device__ __forceinline__ bool edge_ends(int e, const int* __restrict__ n_edges, int V, const int* __restrict__ euv, int& u, int& v)
{
    if (e >= *n_edges) return false;
    u = euv[2 * (size_t)e];
    v = euv[2 * (size_t)e + 1];
    return (unsigned)u < (unsigned)V && (unsigned)v < (unsigned)V;
}

// m1[v] = the smallest key among the candidate edges at v
__global__ void __launch_bounds__(RM_BLOCK) remesh_min1_kernel(int cap, const int* __restrict__ n_edges, int V, const int* __restrict__ euv,
                                                               const long long* __restrict__ key, long long* __restrict__ m1)
{
    const int e = blockIdx.x * RM_BLOCK + threadIdx.x;
    int u, v;
    if (e >= cap || !edge_ends(e, n_edges, V, euv, u, v)) return;
    const long long k = key[e];
    if (k == RM_SENTINEL) return;
    atomicMin(m1 + u, k);
    atomicMin(m1 + v, k);
}

// m2[v] = the smallest m1 over v and its neighbours, along EVERY edge of the mesh
__global__ void __launch_bounds__(RM_BLOCK) remesh_min2_kernel(int cap, const int* __restrict__ n_edges, int V, const int* __restrict__ euv,
                                                               const long long* __restrict__ m1, long long* __restrict__ m2)
{
    const int e = blockIdx.x * RM_BLOCK + threadIdx.x;
    int u, v;
    if (e >= cap || !edge_ends(e, n_edges, V, euv, u, v)) return;
    const long long a = m1[u], b = m1[v], m = a < b ? a : b;
    if (m == RM_SENTINEL) return;
    atomicMin(m2 + u, m);
    atomicMin(m2 + v, m);
}

__global__ void __launch_bounds__(RM_BLOCK) remesh_pick_kernel(int cap, const int* __restrict__ n_edges, int V, const int* __restrict__ euv,
                                                               const long long* __restrict__ key, const long long* __restrict__ m2,
                                                               long long* __restrict__ selected)
{
    const int e = blockIdx.x * RM_BLOCK + threadIdx.x;
    if (e >= cap) return;
    int u, v;
    long long s = RM_SENTINEL;
    if (edge_ends(e, n_edges, V, euv, u, v)) {
        const long long k = key[e];
        if (k != RM_SENTINEL && m2[u] == k && m2[v] == k) s = k;
    }
    selected[e] = s;
}

// ---------------------------------------------------------------------------------------------------- apply
__device__ __forceinline__ bool applied(int e, const int* __restrict__ n_edges, const long long* __restrict__ selected,
                                        const long long* __restrict__ threshold)
{
    if (e >= *n_edges) return false;
    const long long k = selected[e];
    return k != RM_SENTINEL && k <= *threshold;
}

// u survives at the placement with Q_u + Q_v; the edge's two faces die; v becomes u in v's other faces.  No face touches two
// selected edges, so every face and vertex written here is this thread's alone.
__global__ void __launch_bounds__(RM_BLOCK) remesh_apply_kernel(int cap, const int* __restrict__ n_edges, int V, VertexFaces vf,
                                                                const long long* __restrict__ selected, const long long* __restrict__ threshold,
                                                                const int* __restrict__ euv, const double* __restrict__ placement,
                                                                int* __restrict__ faces, int* __restrict__ live, double* __restrict__ pos,
                                                                double* __restrict__ Q)
{
    const int e = blockIdx.x * RM_BLOCK + threadIdx.x;
    if (e >= cap || !applied(e, n_edges, selected, threshold)) return;
    const int u = euv[2 * (size_t)e], v = euv[2 * (size_t)e + 1];
    if ((unsigned)u >= (unsigned)V || (unsigned)v >= (unsigned)V) return;
    for (int t = 0; t < 10; ++t) Q[10 * (size_t)u + t] = Q[10 * (size_t)u + t] + Q[10 * (size_t)v + t];
    for (int k = 0; k < 3; ++k) pos[3 * (size_t)u + k] = placement[3 * (size_t)e + k];
    for (int i = vf.begin(v); i < vf.end(v); ++i) {
        const int f = vf.face(v, i);
        if (f < 0) continue;
        int* c = faces + 3 * (size_t)f;
        if (c[0] == u || c[1] == u || c[2] == u) {
            live[f] = 0;
        } else {
            for (int k = 0; k < 3; ++k)
                if (c[k] == v) c[k] = u;
        }
    }
}

__global__ void __launch_bounds__(RM_BLOCK) remesh_attr_kernel(int cap, const int* __restrict__ n_edges, int V, int C,
                                                               const long long* __restrict__ selected, const long long* __restrict__ threshold,
                                                               const int* __restrict__ euv, float* __restrict__ attr)
{
    const int e = blockIdx.x * RM_BLOCK + threadIdx.x;
    if (e >= cap || !applied(e, n_edges, selected, threshold)) return;
    const int u = euv[2 * (size_t)e], v = euv[2 * (size_t)e + 1];
    if ((unsigned)u >= (unsigned)V || (unsigned)v >= (unsigned)V) return;
    float* au = attr + (size_t)C * u;
    const float* av = attr + (size_t)C * v;
    for (int k = 0; k < C; ++k) au[k] = (au[k] + av[k]) * 0.5f;
}

// ---------------------------------------------------------------------------------------------------- smoothing
// new = prev + lambda (sum w_n prev_n / sum w_n - prev) over the neighbours in ascending order; w_n = 1 / (|prev - prev_n| + 1e-12)
// or 1.  A vertex without neighbours or under `locked` keeps its position.
__global__ void __launch_bounds__(RM_BLOCK) remesh_smooth_kernel(int V, const int* __restrict__ off, const int* __restrict__ nbr,
                                                                 const unsigned char* __restrict__ locked, double lambda, int uniform,
                                                                 const double* __restrict__ in, double* __restrict__ out)
{
    const int v = blockIdx.x * RM_BLOCK + threadIdx.x;
    if (v >= V) return;
    const D3 p = load3(in, (size_t)v);
    D3 r = p;
    const int b = off[v], e = off[v + 1];
    if (e > b && !(locked && locked[v])) {
        double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
        for (int i = b; i < e; ++i) {
            const int n = nbr[i];
            if ((unsigned)n >= (unsigned)V) continue;
            const D3 q = load3(in, (size_t)n);
            double w = 1.0;
            if (!uniform) {
                const D3 d = sub3(p, q);
                w = 1.0 / (sqrt(dot3(d, d)) + 1e-12);
            }
            sx += w * q.x; sy += w * q.y; sz += w * q.z;
            sw += w;
        }
        r = {p.x + lambda * (sx / sw - p.x), p.y + lambda * (sy / sw - p.y), p.z + lambda * (sz / sw - p.z)};
    }
    out[3 * (size_t)v] = r.x;
    out[3 * (size_t)v + 1] = r.y;
    out[3 * (size_t)v + 2] = r.z;
}

inline VertexFaces vertex_faces(int F, const int* off, const long long* corners) { return {off, corners, 3 * (long long)F}; }

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

int gsr_remesh_setup(int F, int V, const float* verts, const int* faces, double* pos, int* live, double* face_quadric, int* err,
                     gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || F <= 0 || V <= 0) return fail_msg("gsr_remesh_setup: sizes must be positive and F at most (2^31 - 1) / 3");
    if (!verts || !faces || !pos || !live || !face_quadric || !err) return fail_msg("gsr_remesh_setup: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    remesh_widen_kernel<<<mesh_blocks(3ll * V), RM_BLOCK, 0, st>>>(3ll * V, verts, pos);
    remesh_face_quadric_kernel<<<mesh_blocks(F), RM_BLOCK, 0, st>>>(F, V, faces, pos, live, face_quadric, err);
    GSR_CHECK_LAUNCH("remesh setup kernels");
    return 0;
}

int gsr_remesh_keys(int F, int V, const int* faces, const int* live, long long* edge_keys, long long* corner_keys, int* degree,
                    gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || F <= 0 || V <= 0) return fail_msg("gsr_remesh_keys: sizes must be positive and F at most (2^31 - 1) / 3");
    if (!faces || !live || !edge_keys || !corner_keys || !degree) return fail_msg("gsr_remesh_keys: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    GSR_CHECK(hipMemsetAsync(degree, 0, sizeof(int) * (size_t)V, st));
    remesh_key_kernel<<<mesh_blocks(F), RM_BLOCK, 0, st>>>(F, V, faces, live, edge_keys, corner_keys, degree);
    GSR_CHECK_LAUNCH("remesh_key_kernel");
    return 0;
}

int gsr_remesh_vertex_quadrics(int F, int V, const int* vf_offsets, const long long* corners, const double* face_quadric, double* quadric,
                               gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || F <= 0 || V <= 0) return fail_msg("gsr_remesh_vertex_quadrics: sizes must be positive and F at most (2^31 - 1) / 3");
    if (!vf_offsets || !corners || !face_quadric || !quadric) return fail_msg("gsr_remesh_vertex_quadrics: required pointer is null");
    remesh_vertex_quadric_kernel<<<mesh_blocks(V), RM_BLOCK, 0, (hipStream_t)stream>>>(V, vertex_faces(F, vf_offsets, corners), face_quadric,
                                                                                       quadric);
    GSR_CHECK_LAUNCH("remesh_vertex_quadric_kernel");
    return 0;
}

int gsr_remesh_edge_heads(int n, const long long* sorted_keys, int* head, gsr_stream_t stream)
{
    clear_error();
    if (n <= 0) return fail_msg("gsr_remesh_edge_heads: n must be positive");
    if (!sorted_keys || !head) return fail_msg("gsr_remesh_edge_heads: required pointer is null");
    remesh_head_kernel<<<mesh_blocks(n), RM_BLOCK, 0, (hipStream_t)stream>>>(n, sorted_keys, head);
    GSR_CHECK_LAUNCH("remesh_head_kernel");
    return 0;
}

int gsr_remesh_edges(int n, int V, const long long* sorted_keys, const long long* order, const int* head_scan, int* edge_verts,
                     unsigned char* manifold, unsigned char* fixed, gsr_stream_t stream)
{
    clear_error();
    if (n <= 0 || V <= 0) return fail_msg("gsr_remesh_edges: sizes must be positive");
    if (!sorted_keys || !order || !head_scan || !edge_verts || !manifold || !fixed) return fail_msg("gsr_remesh_edges: required pointer is null");
    remesh_edge_kernel<<<mesh_blocks(n), RM_BLOCK, 0, (hipStream_t)stream>>>(n, V, sorted_keys, order, head_scan, edge_verts, manifold, fixed);
    GSR_CHECK_LAUNCH("remesh_edge_kernel");
    return 0;
}

int gsr_remesh_candidates(int cap, const int* n_edges, int F, int V, const int* edge_verts, const unsigned char* manifold,
                          const unsigned char* fixed, const int* vf_offsets, const long long* corners, const int* faces, const double* pos,
                          const double* quadric, long long* key, double* placement, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || cap <= 0 || F <= 0 || V <= 0) return fail_msg("gsr_remesh_candidates: sizes must be positive and F at most (2^31 - 1) / 3");
    if (!n_edges || !edge_verts || !manifold || !fixed || !vf_offsets || !corners || !faces || !pos || !quadric || !key || !placement)
        return fail_msg("gsr_remesh_candidates: required pointer is null");
    remesh_candidate_kernel<<<mesh_blocks(cap), RM_BLOCK, 0, (hipStream_t)stream>>>(cap, n_edges, V, vertex_faces(F, vf_offsets, corners),
                                                                                    edge_verts, manifold, fixed, faces, pos, quadric, key,
                                                                                    placement);
    GSR_CHECK_LAUNCH("remesh_candidate_kernel");
    return 0;
}

int gsr_remesh_select(int cap, const int* n_edges, int V, const int* edge_verts, const long long* key, long long* m1, long long* m2,
                      long long* selected, gsr_stream_t stream)
{
    clear_error();
    if (cap <= 0 || V <= 0) return fail_msg("gsr_remesh_select: sizes must be positive");
    if (!n_edges || !edge_verts || !key || !m1 || !m2 || !selected) return fail_msg("gsr_remesh_select: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    remesh_fill_kernel<<<mesh_blocks(V), RM_BLOCK, 0, st>>>(V, m1, m2);
    remesh_min1_kernel<<<mesh_blocks(cap), RM_BLOCK, 0, st>>>(cap, n_edges, V, edge_verts, key, m1);
    remesh_min2_kernel<<<mesh_blocks(cap), RM_BLOCK, 0, st>>>(cap, n_edges, V, edge_verts, m1, m2);
    remesh_pick_kernel<<<mesh_blocks(cap), RM_BLOCK, 0, st>>>(cap, n_edges, V, edge_verts, key, m2, selected);
    GSR_CHECK_LAUNCH("remesh select kernels");
    return 0;
}

int gsr_remesh_cap(int live_faces, int target_faces, int n_selected, int* n_apply)
{
    clear_error();
    if (!n_apply) return fail_msg("gsr_remesh_cap: required pointer is null");
    *n_apply = 0;
    if (live_faces < 0 || n_selected < 0) return fail_msg("gsr_remesh_cap: negative size");
    if (target_faces < 0) return fail_msg("gsr_remesh_cap: target_faces must not be negative");
    if (live_faces <= target_faces) return 0;
    const long long want = ((long long)live_faces - target_faces + 1) / 2;
    *n_apply = (int)(want < n_selected ? want : n_selected);
    return 0;
}

int gsr_remesh_apply(int cap, const int* n_edges, int F, int V, const long long* selected, const long long* threshold, const int* edge_verts,
                     const double* placement, const int* vf_offsets, const long long* corners, int* faces, int* live, double* pos,
                     double* quadric, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || cap <= 0 || F <= 0 || V <= 0) return fail_msg("gsr_remesh_apply: sizes must be positive and F at most (2^31 - 1) / 3");
    if (!n_edges || !selected || !threshold || !edge_verts || !placement || !vf_offsets || !corners || !faces || !live || !pos || !quadric)
        return fail_msg("gsr_remesh_apply: required pointer is null");
    remesh_apply_kernel<<<mesh_blocks(cap), RM_BLOCK, 0, (hipStream_t)stream>>>(cap, n_edges, V, vertex_faces(F, vf_offsets, corners), selected,
                                                                                threshold, edge_verts, placement, faces, live, pos, quadric);
    GSR_CHECK_LAUNCH("remesh_apply_kernel");
    return 0;
}

int gsr_remesh_apply_attr(int cap, const int* n_edges, int V, int C, const long long* selected, const long long* threshold,
                          const int* edge_verts, float* attr, gsr_stream_t stream)
{
    clear_error();
    if (cap <= 0 || V <= 0 || C <= 0) return fail_msg("gsr_remesh_apply_attr: sizes must be positive");
    if (!n_edges || !selected || !threshold || !edge_verts || !attr) return fail_msg("gsr_remesh_apply_attr: required pointer is null");
    remesh_attr_kernel<<<mesh_blocks(cap), RM_BLOCK, 0, (hipStream_t)stream>>>(cap, n_edges, V, C, selected, threshold, edge_verts, attr);
    GSR_CHECK_LAUNCH("remesh_attr_kernel");
    return 0;
}

int gsr_remesh_narrow(long long n, const double* in, float* out, gsr_stream_t stream)
{
    clear_error();
    if (n <= 0) return fail_msg("gsr_remesh_narrow: n must be positive");
    if (!in || !out) return fail_msg("gsr_remesh_narrow: required pointer is null");
    remesh_narrow_kernel<<<mesh_blocks(n), RM_BLOCK, 0, (hipStream_t)stream>>>(n, in, out);
    GSR_CHECK_LAUNCH("remesh_narrow_kernel");
    return 0;
}

int gsr_remesh_smooth(int V, const int* nbr_offsets, const int* nbr, const unsigned char* locked, int steps, double lambda_even,
                      double lambda_odd, int uniform, const float* verts, double* work_a, double* work_b, float* out, gsr_stream_t stream)
{
    clear_error();
    if (V <= 0) return fail_msg("gsr_remesh_smooth: V must be positive");
    if (steps < 0) return fail_msg("gsr_remesh_smooth: steps must not be negative");
    if (!nbr_offsets || !verts || !work_a || !work_b || !out) return fail_msg("gsr_remesh_smooth: required pointer is null");
    if (steps > 0 && !nbr) return fail_msg("gsr_remesh_smooth: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    remesh_widen_kernel<<<mesh_blocks(3ll * V), RM_BLOCK, 0, st>>>(3ll * V, verts, work_a);
    double* src = work_a;
    double* dst = work_b;
    for (int s = 0; s < steps; ++s) {
        remesh_smooth_kernel<<<mesh_blocks(V), RM_BLOCK, 0, st>>>(V, nbr_offsets, nbr, locked, (s & 1) ? lambda_odd : lambda_even, uniform, src,
                                                                  dst);
        double* t = src; src = dst; dst = t;
    }
    remesh_narrow_kernel<<<mesh_blocks(3ll * V), RM_BLOCK, 0, st>>>(3ll * V, src, out);
    GSR_CHECK_LAUNCH("remesh smooth kernels");
    return 0;
}

}  // extern "C"
