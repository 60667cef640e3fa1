// gsr_mesh_lap.hip -- the two surface losses of a refinement iteration that gsr_mesh_reg.hip leaves out, fused: the mesh
// Laplacian-smoothing loss (gaustar_trainers/refine.py:681-683) and the small-area regulariser (refine.py:713-718).
//
// Reference: pytorch3d.loss.mesh_laplacian_smoothing(mesh, method) with pytorch3d.ops.laplacian / cot_laplacian (0.7) for ONE
// mesh, and `relu(mean_area / faces_areas_packed() - 2).mean()` with the mean under no_grad.  The rules are restated in
// include/gsr.h from memory of those sources; parity with pytorch3d itself is not pinned (it is not installed where this
// was written).  pytorch3d builds a sparse V x V matrix per call and multiplies; here nothing per edge is stored: a vertex
// gathers over its own lists, built once per face tensor (gaustar_amd/meshes.py MeshTopology.vertex_neighbours -- ascending
// neighbours -- and vertex_face_csr -- face * 3 + corner ascending).  At vertex i an incident face with the other corners
// j, k adds cot_k v_j + cot_j v_k to the weighted sum and cot_k + cot_j to S_i.
//   forward   face pass (cot methods: three cotangents + Heron area per face, f64; area regulariser: the cross-product area's
//             partial sums) -> area-regulariser face pass (every workgroup totals the partials in the same fixed order, so
//             the mean is on the device without a launch of its own) -> vertex pass (l_i, |l_i|, and what the backward
//             gathers: g_i = c_i u_i and the diagonal d_i u_i) -> single-workgroup finalise -> loss_out[3].
//   backward  ONE vertex-major launch: the same gather with g in place of v, plus the diagonal, plus the area regulariser's
//             contributions over the vertex's faces.
// Weights are constants: no gradient through deg, the cotangents, the areas or the mean area.  The Laplacian path is f64 from
// the f32 positions (l_i is a small difference of nearby positions: in f32 its direction is lost and the gradient misses
// 1e-4 of its largest magnitude), rounded to f32 once at the end; the area regulariser is f32 with f64 sums.  No float
// atomics, no scratch: two calls give identical bits.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_reduce.h"
#include "gsr_v3.h"
#include <cstdio>

namespace gsr {

namespace {

constexpr int ML_UNIFORM = 0, ML_COT = 1, ML_COTCURV = 2;
constexpr double ML_HERON_MIN = 1e-12;   // pytorch3d cot_laplacian: area = sqrt(clamp(s (s-A) (s-B) (s-C), min = 1e-12))

// (contracted, unlike gsr_surface.h's D3: the f64 Laplacian path was written and pinned with the build's default)
struct D3 { double x, y, z; };
__device__ __forceinline__ D3 ld3d(const float* __restrict__ v, int i) { return D3{(double)v[3 * i], (double)v[3 * i + 1], (double)v[3 * i + 2]}; }
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double norm(D3 a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ void axpy(D3& s, double a, D3 v) { s.x += a * v.x; s.y += a * v.y; s.z += a * v.z; }

}  // namespace

struct MeshLapArgs {
    int V, F, method;
    int use_lap, use_areg;
    const float* verts;    // [V,3]
    const int* faces;      // [F,3]
    const int* nbr_off;    // [V+1]   MeshTopology.vertex_neighbours
    const int* nbr;
    const int* vf_off;     // [V+1]   MeshTopology.vertex_face_csr, entry = face * 3 + corner
    const int* vf;         // [3F]
    // workspace
    double* p_area;        // partials of the face pass: sum of cross-product areas
    double* p_lap;         // partials of the vertex pass: sum of |l_i|
    double* p_areg;        // partials of the area-regulariser pass
    float* mean_area;      // [1]
    double* vtx;           // [V,6]  g_i = c_i u_i, then d_i u_i
    double* fc;            // [F,4]  cot_a, cot_b, cot_c, Heron area
};

namespace {

struct WsLayout { size_t p_area, p_lap, p_areg, scal, vtx, fc, total; };

WsLayout ws_layout(int V, int F)
{
    WsLayout w{};
    const size_t part = align_up(RED_STRIDE * sizeof(double) * RED_MAX_WGS);
    size_t o = 0;
    w.p_area = o; o += part;
    w.p_lap = o; o += part;
    w.p_areg = o; o += part;
    w.scal = o; o += 256;
    w.vtx = o; o += align_up((size_t)(V > 0 ? V : 0) * 6 * sizeof(double));
    w.fc = o; o += align_up((size_t)(F > 0 ? F : 0) * 4 * sizeof(double));
    w.total = o + 256;
    return w;
}

__device__ __forceinline__ float cross_area(const MeshLapArgs& m, int f, V3* u, V3* w, V3* c, float* len)
{
    const V3 p0 = ld3(m.verts, m.faces[3 * f]);
    *u = sub(ld3(m.verts, m.faces[3 * f + 1]), p0);
    *w = sub(ld3(m.verts, m.faces[3 * f + 2]), p0);
    *c = cross(*u, *w);
    *len = sqrtf(dot(*c, *c));
    return 0.5f * *len;
}

// the regulariser's term of face f: relu(mean / area - 2)  (+inf at area 0, as the torch composition)
__device__ __forceinline__ float areg_term(float mean, float area) { return fmaxf(mean / area - 2.f, 0.f); }

__global__ void __launch_bounds__(RED_BLOCK)
mesh_lap_face_kernel(MeshLapArgs m, int want_cot)
{
    double s[1] = {0.0};
    for (int f = (int)(blockIdx.x * RED_BLOCK + threadIdx.x); f < m.F; f += (int)(gridDim.x * RED_BLOCK)) {
        if (want_cot) {
            const D3 pa = ld3d(m.verts, m.faces[3 * f]), pb = ld3d(m.verts, m.faces[3 * f + 1]), pc = ld3d(m.verts, m.faces[3 * f + 2]);
            const double A = norm(sub(pb, pc)), B = norm(sub(pa, pc)), C = norm(sub(pa, pb));
            const double h = 0.5 * (A + B + C);
            const double area = sqrt(fmax(h * (h - A) * (h - B) * (h - C), ML_HERON_MIN));
            const double A2 = A * A, B2 = B * B, C2 = C * C;
            double* o = m.fc + 4 * (size_t)f;
            o[0] = (B2 + C2 - A2) / area / 4.0;
            o[1] = (A2 + C2 - B2) / area / 4.0;
            o[2] = (A2 + B2 - C2) / area / 4.0;
            o[3] = area;
        }
        if (m.use_areg) {
            V3 u, w, c; float len;
            s[0] += (double)cross_area(m, f, &u, &w, &c, &len);
        }
    }
    if (m.use_areg) block_partials(s, m.p_area);   // (use_areg: the same in every lane -- the barrier inside is uniform)
}

__global__ void __launch_bounds__(RED_BLOCK)
mesh_lap_areg_kernel(MeshLapArgs m, int n_wg_face)
{
    __shared__ float mean_s;
    double tot[1];   // (defined in thread 0 only)
    tree_total(n_wg_face, m.p_area, tot);
    if (threadIdx.x == 0) {
        mean_s = (float)(tot[0] / (double)m.F);
        if (blockIdx.x == 0) *m.mean_area = mean_s;   // the backward reads it
    }
    __syncthreads();
    const float mean = mean_s;
    double s[1] = {0.0};
    for (int f = (int)(blockIdx.x * RED_BLOCK + threadIdx.x); f < m.F; f += (int)(gridDim.x * RED_BLOCK)) {
        V3 u, w, c; float len;
        s[0] += (double)areg_term(mean, cross_area(m, f, &u, &w, &c, &len));
    }
    block_partials(s, m.p_areg);
}

// the weighted gather at vertex i over its faces: sum += cot_k x_j + cot_j x_k, S += cot_k + cot_j, area += Heron area, where
// x is the f32 positions (X = nullptr) or rows of six doubles (the backward's g)
__device__ __forceinline__ void cot_gather(const MeshLapArgs& m, int i, const double* __restrict__ X, D3& sum, double& S, double& area)
{
    for (int e = m.vf_off[i]; e < m.vf_off[i + 1]; e++) {
        const int code = m.vf[e];
        const int f = code / 3, c = code - 3 * f;
        const int cj = c == 2 ? 0 : c + 1, ck = c == 0 ? 2 : c - 1;
        const int j = m.faces[3 * f + cj], k = m.faces[3 * f + ck];
        const double* q = m.fc + 4 * (size_t)f;
        const double cotj = q[cj], cotk = q[ck];
        const D3 xj = X ? D3{X[6 * (size_t)j], X[6 * (size_t)j + 1], X[6 * (size_t)j + 2]} : ld3d(m.verts, j);
        const D3 xk = X ? D3{X[6 * (size_t)k], X[6 * (size_t)k + 1], X[6 * (size_t)k + 2]} : ld3d(m.verts, k);
        axpy(sum, cotk, xj);
        axpy(sum, cotj, xk);
        S += cotk + cotj;
        area += q[3];
    }
}

__global__ void __launch_bounds__(RED_BLOCK)
mesh_lap_vertex_kernel(MeshLapArgs m)
{
    double s[1] = {0.0};
    for (int i = (int)(blockIdx.x * RED_BLOCK + threadIdx.x); i < m.V; i += (int)(gridDim.x * RED_BLOCK)) {
        const D3 vi = ld3d(m.verts, i);
        D3 sum{0.0, 0.0, 0.0}, l;
        double c, d;   // l_i = c (sum_j W_ij v_j) + d v_i; g = c u (uniform: the 1 / deg of W folded in), diagonal = d u
        if (m.method == ML_UNIFORM) {
            const int a = m.nbr_off[i], b = m.nbr_off[i + 1];
            for (int e = a; e < b; e++) axpy(sum, 1.0, ld3d(m.verts, m.nbr[e]));
            c = b > a ? 1.0 / (double)(b - a) : 0.0;
            d = -1.0;
        } else {
            double S = 0.0, area = 0.0;
            cot_gather(m, i, nullptr, sum, S, area);
            if (m.method == ML_COT) {
                c = S > 0.0 ? 1.0 / S : S;   // pytorch3d leaves a non-positive row sum as it is
                d = -1.0;
            } else {
                c = area > 0.0 ? 0.25 / area : 0.0;
                d = -c * S;
            }
        }
        l = D3{c * sum.x + d * vi.x, c * sum.y + d * vi.y, c * sum.z + d * vi.z};
        const double len = norm(l);
        s[0] += len;
        const double inv = len > 0.0 ? 1.0 / len : 0.0;   // torch's norm backward: 0 at 0
        const D3 u{l.x * inv, l.y * inv, l.z * inv};
        double* o = m.vtx + 6 * (size_t)i;
        o[0] = c * u.x; o[1] = c * u.y; o[2] = c * u.z;
        o[3] = d * u.x; o[4] = d * u.y; o[5] = d * u.z;
    }
    block_partials(s, m.p_lap);
}

__global__ void __launch_bounds__(RED_BLOCK)
mesh_lap_finalize_kernel(MeshLapArgs m, int n_wg_vertex, int n_wg_areg, float laplacian_factor, float area_reg_factor,
                         float* __restrict__ out)
{
    double lap[1] = {0.0}, ar[1] = {0.0};   // (defined in thread 0 only)
    if (m.use_lap) tree_total(n_wg_vertex, m.p_lap, lap);
    if (m.use_areg) tree_total(n_wg_areg, m.p_areg, ar);
    if (threadIdx.x == 0) {
        const float a = m.use_lap ? (float)((double)laplacian_factor * (lap[0] / (double)m.V)) : 0.f;
        const float b = m.use_areg ? (float)((double)area_reg_factor * (ar[0] / (double)m.F)) : 0.f;
        out[0] = a; out[1] = b;
        out[2] = a + b;   // refine.py:683, :718: the trainer's order
    }
}

__global__ void __launch_bounds__(RED_BLOCK)
mesh_lap_bwd_kernel(MeshLapArgs m, float laplacian_factor, float area_reg_factor, const float* __restrict__ scale,
                    float* __restrict__ grad, int accumulate)
{
    const int k = (int)(blockIdx.x * RED_BLOCK + threadIdx.x);
    if (k >= m.V) return;
    D3 g{0.0, 0.0, 0.0};
    if (m.use_lap) {
        // d loss / d v_k = (1 / V) (sum_i c_i W_ik u_i + d_k u_k)
        if (m.method == ML_UNIFORM) {
            for (int e = m.nbr_off[k]; e < m.nbr_off[k + 1]; e++) {
                const double* q = m.vtx + 6 * (size_t)m.nbr[e];
                g.x += q[0]; g.y += q[1]; g.z += q[2];
            }
        } else {
            double S = 0.0, area = 0.0;
            cot_gather(m, k, m.vtx, g, S, area);
        }
        const double* q = m.vtx + 6 * (size_t)k;
        const double f = (double)laplacian_factor / (double)m.V;
        g = D3{f * (g.x + q[3]), f * (g.y + q[4]), f * (g.z + q[5])};
    }
    if (m.use_areg) {
        const float mean = *m.mean_area;
        const float cf = area_reg_factor / (float)m.F;
        V3 a{0.f, 0.f, 0.f};
        for (int e = m.vf_off[k]; e < m.vf_off[k + 1]; e++) {
            const int code = m.vf[e];
            const int f = code / 3, corner = code - 3 * f;
            V3 u, w, c; float len;
            const float area = cross_area(m, f, &u, &w, &c, &len);
            // a zero-area face contributes no gradient (the torch composition gives NaN there: a stated departure)
            if (!(area > 0.f) || !(mean / area > 2.f)) continue;
            const float coef = -cf * mean / (area * area);
            const V3 gc = mul(0.5f * coef / len, c);
            const V3 gu = cross(w, gc), gw = cross(gc, u);
            const V3 t = corner == 1 ? gu : corner == 2 ? gw : mul(-1.f, add(gu, gw));
            a = add(a, t);
        }
        g.x += (double)a.x; g.y += (double)a.y; g.z += (double)a.z;
    }
    {
        // exactly two roundings after the one to f32, never contracted: scale * g, then (with accumulate) X + that
#pragma clang fp contract(off)
        const float s = scale ? *scale : 1.f;
        float* o = grad + 3 * (size_t)k;
        const float gx = s * (float)g.x, gy = s * (float)g.y, gz = s * (float)g.z;
        if (accumulate) { o[0] = o[0] + gx; o[1] = o[1] + gy; o[2] = o[2] + gz; }
        else { o[0] = gx; o[1] = gy; o[2] = gz; }
    }
}

MeshLapArgs make_args(int V, int F, const float* verts, const int* faces, const int* nbr_off, const int* nbr, const int* vf_off,
                      const int* vf, int method, float laplacian_factor, float area_reg_factor, void* workspace)
{
    MeshLapArgs m{};
    m.V = V; m.F = F; m.method = method;
    m.use_lap = laplacian_factor != 0.f && V > 0;
    m.use_areg = area_reg_factor != 0.f && F > 0;
    m.verts = verts; m.faces = faces; m.nbr_off = nbr_off; m.nbr = nbr; m.vf_off = vf_off; m.vf = vf;
    const WsLayout w = ws_layout(V, F);
    char* base = static_cast<char*>(workspace);
    m.p_area = reinterpret_cast<double*>(base + w.p_area);
    m.p_lap = reinterpret_cast<double*>(base + w.p_lap);
    m.p_areg = reinterpret_cast<double*>(base + w.p_areg);
    m.mean_area = reinterpret_cast<float*>(base + w.scal);
    m.vtx = reinterpret_cast<double*>(base + w.vtx);
    m.fc = reinterpret_cast<double*>(base + w.fc);
    return m;
}

int mesh_lap_check(const char* fn, int V, int F, const float* verts, const int* faces, const int* nbr_off, const int* nbr,
                   const int* vf_off, const int* vf, int method, const void* workspace)
{
    char msg[160];
    if (V < 0 || F < 0) { snprintf(msg, sizeof msg, "%s: negative size", fn); return fail_msg(msg); }
    if ((long long)F >= (1ll << 29) || (long long)V >= (1ll << 29)) { snprintf(msg, sizeof msg, "%s: mesh too large", fn); return fail_msg(msg); }
    if (method != ML_UNIFORM && method != ML_COT && method != ML_COTCURV) {
        snprintf(msg, sizeof msg, "%s: method must be 0 (uniform), 1 (cot) or 2 (cotcurv)", fn);
        return fail_msg(msg);
    }
    if (!workspace || (V > 0 && (!verts || !nbr_off || !vf_off)) || (F > 0 && (V <= 0 || !faces || !nbr || !vf))) {
        snprintf(msg, sizeof msg, "%s: required pointer is null", fn);
        return fail_msg(msg);
    }
    if (reinterpret_cast<uintptr_t>(workspace) & 7) { snprintf(msg, sizeof msg, "%s: workspace must be 8-byte aligned", fn); return fail_msg(msg); }
    return 0;
}

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

size_t gsr_mesh_lap_workspace_bytes(int V, int F)
{
    return ws_layout(V, F).total;
}

int gsr_mesh_lap_forward(int V, int F, const float* verts, const int* faces, const int* nbr_offsets, const int* nbr,
                         const int* vf_offsets, const int* vf_entries, int method, float laplacian_factor, float area_reg_factor,
                         void* workspace, float* loss_out, gsr_stream_t stream)
{
    clear_error();
    if (int rc = mesh_lap_check("gsr_mesh_lap_forward", V, F, verts, faces, nbr_offsets, nbr, vf_offsets, vf_entries, method, workspace))
        return rc;
    if (!loss_out) return fail_msg("gsr_mesh_lap_forward: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    {
        Scope sc(ST_LOSS, st);
        const MeshLapArgs m = make_args(V, F, verts, faces, nbr_offsets, nbr, vf_offsets, vf_entries, method, laplacian_factor,
                                        area_reg_factor, workspace);
        const int want_cot = m.use_lap && method != ML_UNIFORM && F > 0;
        const int n_wg_f = reduce_workgroups(F), n_wg_v = reduce_workgroups(V);
        if (want_cot || m.use_areg) mesh_lap_face_kernel<<<n_wg_f, RED_BLOCK, 0, st>>>(m, want_cot);
        if (m.use_areg) mesh_lap_areg_kernel<<<n_wg_f, RED_BLOCK, 0, st>>>(m, n_wg_f);
        if (m.use_lap) mesh_lap_vertex_kernel<<<n_wg_v, RED_BLOCK, 0, st>>>(m);
        mesh_lap_finalize_kernel<<<1, RED_BLOCK, 0, st>>>(m, n_wg_v, n_wg_f, laplacian_factor, area_reg_factor, loss_out);
    }
    GSR_CHECK_LAUNCH("mesh_lap forward kernels");
    return 0;
}

int gsr_mesh_lap_backward(int V, int F, const float* verts, const int* faces, const int* nbr_offsets, const int* nbr,
                          const int* vf_offsets, const int* vf_entries, int method, float laplacian_factor, float area_reg_factor,
                          void* workspace, const float* grad_scale, float* dL_dverts, int accumulate, gsr_stream_t stream)
{
    clear_error();
    if (int rc = mesh_lap_check("gsr_mesh_lap_backward", V, F, verts, faces, nbr_offsets, nbr, vf_offsets, vf_entries, method, workspace))
        return rc;
    if (accumulate != 0 && accumulate != 1) return fail_msg("gsr_mesh_lap_backward: accumulate must be 0 or 1");
    if (V == 0) return 0;
    if (!dL_dverts) return fail_msg("gsr_mesh_lap_backward: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    {
        Scope sc(ST_LOSS, st);
        const MeshLapArgs m = make_args(V, F, verts, faces, nbr_offsets, nbr, vf_offsets, vf_entries, method, laplacian_factor,
                                        area_reg_factor, workspace);
        mesh_lap_bwd_kernel<<<(V + RED_BLOCK - 1) / RED_BLOCK, RED_BLOCK, 0, st>>>(m, laplacian_factor, area_reg_factor, grad_scale,
                                                                                 dL_dverts, accumulate);
    }
    GSR_CHECK_LAUNCH("mesh_lap_bwd_kernel");
    return 0;
}

}  // extern "C"
