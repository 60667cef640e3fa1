// gsr_mesh_reg.hip -- the surface-mesh regularisers of a refinement iteration, fused: normal consistency, edge isometry and
// area isometry (gaustar_trainers/refine.py:676-706).
//
// Reference: pytorch3d.loss.mesh_normal_consistency, `((edge_len - ref_edge_len)**2).mean()` over Meshes.edges_packed() and
// `(faces_areas_packed() - ref_area).abs().mean()`.  pytorch3d rebuilds the face pairs of every edge on each call (a sort of
// the 3F face-edges, bincount, data-dependent shapes: host synchronisations every iteration).  Here the topology -- edges,
// the face pairs of every edge, a vertex-major incidence list -- is built once per face tensor (gaustar_amd/meshes.py) and
// the per-iteration work is two passes over it:
//   forward   one element pass over {pairs, edges, faces} and one single-workgroup finalise, summed in double in a fixed
//             order (gsr_reduce.h) -> loss_out[4] = {nc, edge, area, total};
//   backward  ONE vertex-major pass: a workgroup takes MR_VPB consecutive vertices, its lanes recompute the derivative of
//             every incidence in the vertices' lists (chunks of 256 in LDS), and each vertex's lane sums its own entries in
//             list order.  No float atomics: two calls give identical bits.
//
// Element index space: pairs [0, Q), edges [Q, Q + E), faces [Q + E, Q + E + F).  An incidence entry is elem * 4 + role:
//   pair (e0, e1, a, b): role 0 = e0, 1 = e1, 2 = a, 3 = b;  edge (v0, v1): role 0, 1;  face (v0, v1, v2): role = corner.
//
// Per pair (edge (e0, e1) with the corners a, b of its two faces that are not on it), as pytorch3d:
//   n0 = (e1 - e0) x (a - e0),  n1 = -((e1 - e0) x (b - e0)),  term = 1 - cosine_similarity(n0, n1, eps = 1e-8)
// with torch's cosine_similarity: x / max(|x|, eps) . y / max(|y|, eps), whose gradient through the norm is x / |x| (0 at
// x = 0) even where the clamp is active.  Edge: |v0 - v1|, gradient 0 at length 0.  Face area: 0.5 |(v1 - v0) x (v2 - v0)|
// with torch's d|c|/dc = 0 at c = 0 and d|x|/dx = 0 at x = 0: a degenerate face contributes no area gradient.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_reduce.h"
#include "gsr_v3.h"
#include <cstdio>

namespace gsr {

namespace {

constexpr int MR_BLOCK = 256;       // backward (the forward pair runs RED_BLOCK lanes)
constexpr int MR_VPB = 32;          // backward: vertices per workgroup (config C: ~24 incidences each -> 3 chunks of 256)
constexpr float MR_EPS = 1e-8f;     // torch.nn.functional.cosine_similarity's default eps, as pytorch3d calls it

}  // namespace

struct MeshRegArgs {
    int Q, E, F;
    const float* verts;      // [V,3]
    const int* faces;        // [F,3]
    const int* edges;        // [E,2]
    const int* pairs;        // [Q,4] (e0, e1, a, b)
    const float* ref_edge;   // [E] or null
    const float* ref_area;   // [F] or null
    float cq, ce, ca;        // backward: nc_factor / Q, 2 edge_factor / E, area_factor / F (0: term off)
    int use_nc, use_edge, use_area;
};

namespace {

// 1 - cos(n0, n1) of pair q; with g non-null also its derivative w.r.t. the vertex in `role` (0 e0, 1 e1, 2 a, 3 b)
__device__ __forceinline__ float pair_term(const MeshRegArgs& m, int q, int role, V3* g)
{
    const int4 p = reinterpret_cast<const int4*>(m.pairs)[q];
    const V3 p0 = ld3(m.verts, p.x), p1 = ld3(m.verts, p.y), pa = ld3(m.verts, p.z), pb = ld3(m.verts, p.w);
    const V3 d = sub(p1, p0), wa = sub(pa, p0), wb = sub(pb, p0);
    const V3 n0 = cross(d, wa), n1 = neg(cross(d, wb));
    const float l0 = sqrtf(dot(n0, n0)), l1 = sqrtf(dot(n1, n1));
    const float N0 = fmaxf(l0, MR_EPS), N1 = fmaxf(l1, MR_EPS);
    const float inv = 1.f / (N0 * N1);
    const float cs = dot(n0, n1) * inv;
    if (g) {
        // d(1 - cos)/dn0 = -(n1 / (N0 N1) - cos / (N0 |n0|) n0), the second part only where |n0| > 0 (torch's norm backward)
        const float k0 = l0 > 0.f ? cs / (N0 * l0) : 0.f, k1 = l1 > 0.f ? cs / (N1 * l1) : 0.f;
        const V3 g0 = sub(mul(k0, n0), mul(inv, n1));
        const V3 gm = sub(mul(inv, n0), mul(k1, n1));           // w.r.t. d x wb  (n1 = -(d x wb))
        const V3 ga = cross(g0, d), gb = cross(gm, d);
        const V3 gd = add(cross(wa, g0), cross(wb, gm));
        *g = role == 1 ? gd : role == 2 ? ga : role == 3 ? gb : neg(add(add(gd, ga), gb));
    }
    return 1.f - cs;
}

__device__ __forceinline__ float edge_term(const MeshRegArgs& m, int e, V3* g0)
{
    const int2 ev = reinterpret_cast<const int2*>(m.edges)[e];
    const V3 d = sub(ld3(m.verts, ev.x), ld3(m.verts, ev.y));          // refine.py:693-694: (v0 - v1).norm()
    const float len = sqrtf(dot(d, d));
    const float r = len - m.ref_edge[e];
    if (g0) *g0 = len > 0.f ? mul(m.ce * r / len, d) : V3{0.f, 0.f, 0.f};
    return r * r;
}

__device__ __forceinline__ float area_term(const MeshRegArgs& m, int f, int corner, V3* g)
{
    const int i0 = m.faces[3 * f], i1 = m.faces[3 * f + 1], i2 = m.faces[3 * f + 2];
    const V3 p0 = ld3(m.verts, i0);
    const V3 u = sub(ld3(m.verts, i1), p0), w = sub(ld3(m.verts, i2), p0);
    const V3 c = cross(u, w);
    const float l = sqrtf(dot(c, c));
    const float r = 0.5f * l - m.ref_area[f];
    if (g) {
        const float s = r > 0.f ? m.ca : r < 0.f ? -m.ca : 0.f;       // d|x|/dx = 0 at 0
        const V3 gc = l > 0.f ? mul(0.5f * s / l, c) : V3{0.f, 0.f, 0.f};
        const V3 gu = cross(w, gc), gw = cross(gc, u);
        *g = corner == 1 ? gu : corner == 2 ? gw : neg(add(gu, gw));
    }
    return fabsf(r);
}

__global__ void __launch_bounds__(RED_BLOCK)
mesh_reg_fwd_kernel(MeshRegArgs m, double* __restrict__ partials)
{
    const int N = m.Q + m.E + m.F;
    double s[3] = {0.0, 0.0, 0.0};   // nc, edge, area
    for (int i = (int)(blockIdx.x * RED_BLOCK + threadIdx.x); i < N; i += (int)(gridDim.x * RED_BLOCK)) {
        if (i < m.Q) {
            if (m.use_nc) s[0] += (double)pair_term(m, i, 0, nullptr);
        } else if (i < m.Q + m.E) {
            if (m.use_edge) s[1] += (double)edge_term(m, i - m.Q, nullptr);
        } else if (m.use_area) {
            s[2] += (double)area_term(m, i - m.Q - m.E, 0, nullptr);
        }
    }
    block_partials(s, partials);
}

__global__ void __launch_bounds__(RED_BLOCK)
mesh_reg_finalize_kernel(int n_wg, const double* __restrict__ partials, int Q, int E, int F, float nc_factor, float edge_factor,
                         float area_factor, int use_nc, int use_edge, int use_area, float* __restrict__ out)
{
    double r[3];   // (defined in thread 0 only)
    tree_total(n_wg, partials, r);
    if (threadIdx.x == 0) {
        const float nc = use_nc ? (float)((double)nc_factor * (r[0] / (double)Q)) : 0.f;
        const float ed = use_edge ? (float)((double)edge_factor * (r[1] / (double)E)) : 0.f;
        const float ar = use_area ? (float)((double)area_factor * (r[2] / (double)F)) : 0.f;
        out[0] = nc; out[1] = ed; out[2] = ar;
        out[3] = (nc + ed) + ar;   // refine.py:688, :696, :702: the three additions in the trainer's order
    }
}

__device__ __forceinline__ V3 entry_grad(const MeshRegArgs& m, int code)
{
    const int elem = code >> 2, role = code & 3;
    if (elem < m.Q) {
        if (!m.use_nc) return V3{0.f, 0.f, 0.f};
        V3 g;
        pair_term(m, elem, role, &g);
        return mul(m.cq, g);
    }
    if (elem < m.Q + m.E) {
        if (!m.use_edge) return V3{0.f, 0.f, 0.f};
        V3 g;
        edge_term(m, elem - m.Q, &g);
        return role == 0 ? g : neg(g);
    }
    if (!m.use_area) return V3{0.f, 0.f, 0.f};
    V3 g;
    area_term(m, elem - m.Q - m.E, role, &g);
    return g;
}

__global__ void __launch_bounds__(MR_BLOCK)
mesh_reg_bwd_kernel(MeshRegArgs m, int V, const int* __restrict__ offsets, const int* __restrict__ entries,
                    const float* __restrict__ scale, float* __restrict__ grad, int accumulate)
{
    __shared__ float bx[MR_BLOCK], by[MR_BLOCK], bz[MR_BLOCK];
    const int t = threadIdx.x;
    const int v0 = (int)blockIdx.x * MR_VPB;
    const int nv = min(MR_VPB, V - v0);
    const int k0 = offsets[v0], k1 = offsets[v0 + nv];
    const int lo = t < nv ? offsets[v0 + t] : 0, hi = t < nv ? offsets[v0 + t + 1] : 0;
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int c = k0; c < k1; c += MR_BLOCK) {     // (k0, k1: the same in every lane -- the barriers are uniform)
        V3 g{0.f, 0.f, 0.f};
        if (c + t < k1) g = entry_grad(m, entries[c + t]);
        bx[t] = g.x; by[t] = g.y; bz[t] = g.z;
        __syncthreads();
        const int a = max(lo, c), b = min(hi, c + MR_BLOCK);
        for (int j = a; j < b; j++) { ax += bx[j - c]; ay += by[j - c]; az += bz[j - c]; }   // list order
        __syncthreads();
    }
    if (t < nv) {
        // exactly two roundings, never contracted: scale * sum, then (with accumulate) X + that -- torch's `X + fresh`
#pragma clang fp contract(off)
        const float s = scale ? *scale : 1.f;
        float* o = grad + 3 * (size_t)(v0 + t);
        const float gx = s * ax, gy = s * ay, gz = s * az;
        if (accumulate) { o[0] = o[0] + gx; o[1] = o[1] + gy; o[2] = o[2] + gz; }
        else { o[0] = gx; o[1] = gy; o[2] = gz; }
    }
}

MeshRegArgs make_args(int F, int E, int Q, const float* verts, const int* faces, const int* edges, const int* pairs,
                      const float* ref_edge, const float* ref_area, float nc_factor, float edge_factor, float area_factor)
{
    MeshRegArgs m{};
    m.Q = Q; m.E = E; m.F = F; m.verts = verts; m.faces = faces; m.edges = edges; m.pairs = pairs;
    m.ref_edge = ref_edge; m.ref_area = ref_area;
    m.use_nc = nc_factor != 0.f && Q > 0;
    m.use_edge = edge_factor != 0.f && ref_edge != nullptr && E > 0;
    m.use_area = area_factor != 0.f && ref_area != nullptr && F > 0;
    m.cq = m.use_nc ? (float)((double)nc_factor / (double)Q) : 0.f;
    m.ce = m.use_edge ? (float)(2.0 * (double)edge_factor / (double)E) : 0.f;
    m.ca = m.use_area ? (float)((double)area_factor / (double)F) : 0.f;
    return m;
}

int mesh_reg_check(const char* fn, int V, int F, int E, int Q, const float* verts, const int* faces, const int* edges,
                   const int* pairs)
{
    char msg[160];
    if (V < 0 || F < 0 || E < 0 || Q < 0) { snprintf(msg, sizeof msg, "%s: negative size", fn); return fail_msg(msg); }
    if ((long long)Q + E + F >= (1ll << 29)) { snprintf(msg, sizeof msg, "%s: mesh too large", fn); return fail_msg(msg); }
    if (F > 0 && (V <= 0 || !verts || !faces || !edges || (Q > 0 && !pairs))) {
        snprintf(msg, sizeof msg, "%s: required pointer is null", fn);
        return fail_msg(msg);
    }
    if ((reinterpret_cast<uintptr_t>(pairs) & 15) || (reinterpret_cast<uintptr_t>(edges) & 7)) {
        snprintf(msg, sizeof msg, "%s: pairs must be 16-byte and edges 8-byte aligned", fn);
        return fail_msg(msg);
    }
    return 0;
}

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

size_t gsr_mesh_reg_workspace_bytes(int V, int F, int E, int Q)
{
    (void)V; (void)F; (void)E; (void)Q;   // (the partials of at most 2048 workgroups, whatever the mesh)
    return reduce_workspace_bytes();
}

int gsr_mesh_reg_forward(int V, int F, int E, int Q, const float* verts, const int* faces, const int* edges, const int* pairs,
                         const float* ref_edge_len, const float* ref_area, float nc_factor, float edge_factor, float area_factor,
                         void* workspace, float* loss_out, gsr_stream_t stream)
{
    clear_error();
    if (int rc = mesh_reg_check("gsr_mesh_reg_forward", V, F, E, Q, verts, faces, edges, pairs)) return rc;
    if (!workspace || !loss_out) return fail_msg("gsr_mesh_reg_forward: required pointer is null");
    if (F == 0) E = Q = 0;
    hipStream_t st = (hipStream_t)stream;
    {
        Scope sc(ST_LOSS, st);
        const MeshRegArgs m = make_args(F, E, Q, verts, faces, edges, pairs, ref_edge_len, ref_area, nc_factor, edge_factor, area_factor);
        double* partials = static_cast<double*>(workspace);
        const int n_wg = reduce_workgroups((long long)Q + E + F);
        if (n_wg > 0) mesh_reg_fwd_kernel<<<n_wg, RED_BLOCK, 0, st>>>(m, partials);
        mesh_reg_finalize_kernel<<<1, RED_BLOCK, 0, st>>>(n_wg, partials, Q, E, F, nc_factor, edge_factor, area_factor, m.use_nc,
                                                         m.use_edge, m.use_area, loss_out);
    }
    GSR_CHECK_LAUNCH("mesh_reg forward kernels");
    return 0;
}

int gsr_mesh_reg_backward(int V, int F, int E, int Q, const float* verts, const int* faces, const int* edges, const int* pairs,
                          const int* csr_offsets, const int* csr_entries, const float* ref_edge_len, const float* ref_area,
                          float nc_factor, float edge_factor, float area_factor, const float* grad_scale, float* dL_dverts,
                          int accumulate, gsr_stream_t stream)
{
    clear_error();
    if (int rc = mesh_reg_check("gsr_mesh_reg_backward", V, F, E, Q, verts, faces, edges, pairs)) return rc;
    if (accumulate != 0 && accumulate != 1) return fail_msg("gsr_mesh_reg_backward: accumulate must be 0 or 1");
    if (V == 0) return 0;
    if (!csr_offsets || !csr_entries || !dL_dverts) return fail_msg("gsr_mesh_reg_backward: required pointer is null");
    if (F == 0) E = Q = 0;
    hipStream_t st = (hipStream_t)stream;
    {
        Scope sc(ST_LOSS, st);
        const MeshRegArgs m = make_args(F, E, Q, verts, faces, edges, pairs, ref_edge_len, ref_area, nc_factor, edge_factor, area_factor);
        mesh_reg_bwd_kernel<<<(V + MR_VPB - 1) / MR_VPB, MR_BLOCK, 0, st>>>(m, V, csr_offsets, csr_entries, grad_scale, dL_dverts,
                                                                          accumulate);
    }
    GSR_CHECK_LAUNCH("mesh_reg_bwd_kernel");
    return 0;
}

}  // extern "C"
