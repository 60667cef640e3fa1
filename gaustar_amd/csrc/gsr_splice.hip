// gsr_splice.hip -- what update_mesh_topo (gaustar_trainers/refined_mesh.py:463-693) still needed after the cuts (gsr_regions.hip)
// and the stitch (gsr_stitch.hip): fill_holes (:589, :617, :652) by this project's canonical rule, and the reference areas
// (:683-687) with the mean unique-edge length of force_short_edge (:484-485).
//
// The rule (gaustar_amd.regions.fill_small_holes states it in full).  Boundary face-edges are those of count exactly 1
// (gsr_regions_edge_runs), each with the direction a -> b it has in its face.  Taken undirected they split the vertices they
// touch into components (gsr_unionfind.h: the root is the lowest vertex, m).  A component is a rim iff every one of its vertices
// ends exactly two boundary edges; rims of 3 or 4 vertices are filled, everything else stays.  With x < y the neighbours of m
// on the rim and o the vertex opposite m: a triangle rim gives (m, x, y); a quad rim A = (m, x, o) and B = (o, y, m).  A face
// (a, b, c) is reversed to (a, c, b) iff the boundary edge between its first two vertices runs a -> b in its own face -- the
// triangle and A on the edge m-x, B on the edge o-y, each on its own.  New faces are appended, rims in ascending m, A before B.
// trimesh's fill_holes agrees wherever its answer does not depend on networkx's cycle traversal; it may also fill part of a
// component that has a vertex of degree != 2, which is left alone here.
//
//   rim edges   splice_rim_edge_kernel     per face-edge of count 1: its vertex pair into a dense pair slot, an integer add on the
//                                          degree of each end, and the edge into one of the end's two neighbour slots as
//                                          neighbour << 1 | (the edge leaves this vertex).  The slot order is whatever the adds
//                                          gave; the emit pass orders by x < y, so it shows in no output.
//               uf_init / uf_hook / uf_flatten_kernel (gsr_unionfind.h)
//   census      splice_census_kernel       integer adds at the root: vertices of the component, and a flag `some degree != 2`
//               splice_decide_kernel       per root: 0, 1 or 2 new faces
//               (torch.cumsum of the new faces, one host read of the total)
//   emit        splice_emit_kernel         one thread per root with new faces walks its <= 4 vertices through the slots
//   areas       splice_area_kernel         trimesh's area_faces in float64, contraction off
//               splice_edge_length_kernel  the length of a unique edge from its key, in float64
//               splice_sum / splice_mean_kernel   the mean by the fixed-order reduction of gsr_reduce.h: the same bits every call
// Every value a kernel here reads was written by an earlier launch, except inside the union-find, whose accesses are agent-scope
// atomics.  No float atomics.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_internal.h"
#include "gsr_mesh.h"
#include "gsr_reduce.h"
#include "gsr_unionfind.h"

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int SP_BLOCK = MESH_BLOCK;

// ---------------------------------------------------------------------------------------------------- rim edges
// pairs [3 F]; on [V], degree [V] (zero before); slots [V][2].  A third edge at a vertex only raises its degree.
__global__ void __launch_bounds__(SP_BLOCK) splice_rim_edge_kernel(int F, int V, const int* __restrict__ faces, const int* __restrict__ counts,
                                                                   int2* __restrict__ pairs, unsigned char* __restrict__ on,
                                                                   int* __restrict__ degree, unsigned* __restrict__ slots,
                                                                   int* __restrict__ err)
{
    const int f = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (f >= F) return;
    int v[3];
    const bool ok = mesh_face(faces, f, V, v);
    if (!ok) atomicOr(err, MESH_ERR_INDEX);
    for (int e = 0; e < 3; ++e) {
        int2 pr = make_int2(-1, -1);
        if (ok && counts[3 * (size_t)f + e] == 1) {
            const int a = v[e], b = v[(e + 1) % 3];
            pr = make_int2(a, b);
            on[a] = 1; on[b] = 1;
            const int ka = atomicAdd(degree + a, 1);
            if (ka < 2) slots[2 * (size_t)a + ka] = ((unsigned)b << 1) | 1u;
            const int kb = atomicAdd(degree + b, 1);
            if (kb < 2) slots[2 * (size_t)b + kb] = (unsigned)a << 1;
        }
        pairs[3 * (size_t)f + e] = pr;
    }
}

// ---------------------------------------------------------------------------------------------------- census
// size [V], bad [V] (zero before), at the component's lowest vertex
__global__ void __launch_bounds__(SP_BLOCK) splice_census_kernel(int V, const int* __restrict__ degree, const int* __restrict__ parent,
                                                                 int* __restrict__ size, int* __restrict__ bad)
{
    const int v = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (v >= V) return;
    const int d = degree[v];
    if (d == 0) return;
    const int r = parent[v];
    atomicAdd(size + r, 1);
    if (d != 2) atomicOr(bad + r, 1);
}

__global__ void __launch_bounds__(SP_BLOCK) splice_decide_kernel(int V, const int* __restrict__ degree, const int* __restrict__ parent,
                                                                 const int* __restrict__ size, const int* __restrict__ bad,
                                                                 int* __restrict__ new_faces)
{
    const int v = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (v >= V) return;
    int n = 0;
    if (degree[v] == 2 && parent[v] == v && !bad[v]) n = size[v] == 3 ? 1 : (size[v] == 4 ? 2 : 0);
    new_faces[v] = n;
}

// ---------------------------------------------------------------------------------------------------- emit
__device__ __forceinline__ void put_face(int* __restrict__ o, int a, int b, int c, bool reversed)
{
    o[0] = a; o[1] = reversed ? c : b; o[2] = reversed ? b : c;
}

// scan: the INCLUSIVE scan of new_faces.  A root's component is a simple cycle of 3 or 4 vertices of degree 2 (the census), so
// every slot read here was written and names a vertex of the cycle; the range tests only keep a caller's wrong arrays from
// being indexed with.
__global__ void __launch_bounds__(SP_BLOCK) splice_emit_kernel(int V, int n_new, const int* __restrict__ new_faces, const int* __restrict__ scan,
                                                               const unsigned* __restrict__ slots, int* __restrict__ faces_out,
                                                               int* __restrict__ rim_of_new)
{
    const int m = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (m >= V) return;
    const int nf = new_faces[m];
    if (nf != 1 && nf != 2) return;
    const int k = scan[m] - nf;
    if (k < 0 || k + nf > n_new) return;
    const unsigned s0 = slots[2 * (size_t)m], s1 = slots[2 * (size_t)m + 1];
    const bool first = (s0 >> 1) < (s1 >> 1);
    const unsigned sx = first ? s0 : s1, sy = first ? s1 : s0;
    const int x = (int)(sx >> 1), y = (int)(sy >> 1);
    if ((unsigned)x >= (unsigned)V || (unsigned)y >= (unsigned)V) return;
    const bool m_to_x = (sx & 1u) != 0;
    int* out = faces_out + 3 * (size_t)k;
    rim_of_new[k] = m;
    if (nf == 1) {
        put_face(out, m, x, y, m_to_x);
        return;
    }
    const unsigned t0 = slots[2 * (size_t)x], t1 = slots[2 * (size_t)x + 1];
    const int o = (int)(t0 >> 1) == m ? (int)(t1 >> 1) : (int)(t0 >> 1);
    if ((unsigned)o >= (unsigned)V) return;
    const unsigned u0 = slots[2 * (size_t)o], u1 = slots[2 * (size_t)o + 1];
    const unsigned uy = (int)(u0 >> 1) == y ? u0 : u1;
    put_face(out, m, x, o, m_to_x);
    put_face(out + 3, o, y, m, (uy & 1u) != 0);
    rim_of_new[k + 1] = m;
}

// ---------------------------------------------------------------------------------------------------- areas
__device__ __forceinline__ void load3(const float* __restrict__ verts, int v, double (&p)[3])
{
    for (int a = 0; a < 3; ++a) p[a] = (double)verts[3 * (size_t)v + a];
}

// trimesh's area_faces: u = v1 - v0, w = v2 - v1 (np.diff), c = u x w, area = sqrt((cx cx + cy cy) + cz cz) / 2
__global__ void __launch_bounds__(SP_BLOCK) splice_area_kernel(int F, int V, const int* __restrict__ faces, const float* __restrict__ verts,
                                                               double* __restrict__ area, int* __restrict__ err)
{
    const int f = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (f >= F) return;
    int v[3];
    if (!mesh_face(faces, f, V, v)) {
        atomicOr(err, MESH_ERR_INDEX);
        area[f] = 0.0;
        return;
    }
    double p0[3], p1[3], p2[3];
    load3(verts, v[0], p0); load3(verts, v[1], p1); load3(verts, v[2], p2);
    const double ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
    const double wx = p2[0] - p1[0], wy = p2[1] - p1[1], wz = p2[2] - p1[2];
    const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
    const double s = (cx * cx + cy * cy) + cz * cz;
    area[f] = 0.5 * sqrt(s);
}

// keys [n]: min << 32 | max of a vertex pair (gsr_regions_edge_keys).  length = sqrt((dx dx + dy dy) + dz dz), d = v[min] - v[max]
__global__ void __launch_bounds__(SP_BLOCK) splice_edge_length_kernel(int n, int V, const long long* __restrict__ keys, const float* __restrict__ verts,
                                                                      double* __restrict__ length, int* __restrict__ err)
{
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long k = keys[i];
    const long long a = k >> 32, b = k & 0xffffffffll;
    if (a < 0 || a >= V || b >= V) {
        atomicOr(err, MESH_ERR_INDEX);
        length[i] = 0.0;
        return;
    }
    double p[3], q[3];
    load3(verts, (int)a, p); load3(verts, (int)b, q);
    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    length[i] = sqrt((dx * dx + dy * dy) + dz * dz);
}

// A thread adds x[i], i = its global index, + the grid's size, ... in that order; then gsr_reduce.h's fixed tree.
__global__ void __launch_bounds__(RED_BLOCK) splice_sum_kernel(long long n, const double* __restrict__ x, double* __restrict__ partials)
{
    double s[1] = {0.0};
    const long long stride = (long long)gridDim.x * RED_BLOCK;
    for (long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x; i < n; i += stride) s[0] += x[i];
    block_partials<1>(s, partials);
}

__global__ void __launch_bounds__(RED_BLOCK) splice_mean_kernel(int n_wg, const double* __restrict__ partials, long long n, double* __restrict__ mean)
{
    double t[1];
    tree_total<1>(n_wg, partials, t);
    if (threadIdx.x == 0) mean[0] = t[0] / (double)n;
}

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

size_t gsr_splice_workspace_bytes(void) { return reduce_workspace_bytes(); }

int gsr_splice_rim_edges(int F, int V, const int* faces, const int* counts, int* pairs, unsigned char* on_rim, int* degree,
                         unsigned int* slots, int* parent, int* root_flag, int* err, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || V < 0) return fail_msg("gsr_splice_rim_edges: negative size or too many faces");
    if (V == 0) return 0;
    if (!on_rim || !degree || !slots || !parent || !root_flag || (F > 0 && (!faces || !counts || !pairs || !err)))
        return fail_msg("gsr_splice_rim_edges: required pointer is null");
    if (reinterpret_cast<uintptr_t>(pairs) & 7) return fail_msg("gsr_splice_rim_edges: pairs must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    GSR_CHECK(hipMemsetAsync(on_rim, 0, (size_t)V, st));
    GSR_CHECK(hipMemsetAsync(degree, 0, sizeof(int) * (size_t)V, st));
    GSR_CHECK(hipMemsetAsync(slots, 0xff, 2 * sizeof(unsigned) * (size_t)V, st));
    if (F > 0) splice_rim_edge_kernel<<<mesh_blocks(F), SP_BLOCK, 0, st>>>(F, V, faces, counts, reinterpret_cast<int2*>(pairs), on_rim, degree, slots, err);
    launch_union_find(V, 3ll * F, reinterpret_cast<const int2*>(pairs), on_rim, parent, root_flag, st);
    GSR_CHECK_LAUNCH("splice rim-edge kernels");
    return 0;
}

int gsr_splice_rim_census(int V, const int* degree, const int* parent, int* size, int* bad, int* new_faces, gsr_stream_t stream)
{
    clear_error();
    if (V < 0) return fail_msg("gsr_splice_rim_census: negative size");
    if (V == 0) return 0;
    if (!degree || !parent || !size || !bad || !new_faces) return fail_msg("gsr_splice_rim_census: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    GSR_CHECK(hipMemsetAsync(size, 0, sizeof(int) * (size_t)V, st));
    GSR_CHECK(hipMemsetAsync(bad, 0, sizeof(int) * (size_t)V, st));
    splice_census_kernel<<<mesh_blocks(V), SP_BLOCK, 0, st>>>(V, degree, parent, size, bad);
    splice_decide_kernel<<<mesh_blocks(V), SP_BLOCK, 0, st>>>(V, degree, parent, size, bad, new_faces);
    GSR_CHECK_LAUNCH("splice census kernels");
    return 0;
}

int gsr_splice_rim_emit(int V, int n_new, const int* new_faces, const int* new_scan, const unsigned int* slots, int* faces_out,
                        int* rim_of_new, gsr_stream_t stream)
{
    clear_error();
    if (V < 0 || n_new < 0 || n_new > 0x7fffffff / 3) return fail_msg("gsr_splice_rim_emit: negative size or too many faces");
    if (V == 0 || n_new == 0) return 0;
    if (!new_faces || !new_scan || !slots || !faces_out || !rim_of_new) return fail_msg("gsr_splice_rim_emit: required pointer is null");
    splice_emit_kernel<<<mesh_blocks(V), SP_BLOCK, 0, (hipStream_t)stream>>>(V, n_new, new_faces, new_scan, slots, faces_out, rim_of_new);
    GSR_CHECK_LAUNCH("splice_emit_kernel");
    return 0;
}

int gsr_splice_face_areas(int F, int V, const int* faces, const float* verts, double* area, int* err, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || V < 0) return fail_msg("gsr_splice_face_areas: negative size or too many faces");
    if (F == 0) return 0;
    if (!faces || !area || !err || (V > 0 && !verts)) return fail_msg("gsr_splice_face_areas: required pointer is null");
    splice_area_kernel<<<mesh_blocks(F), SP_BLOCK, 0, (hipStream_t)stream>>>(F, V, faces, verts, area, err);
    GSR_CHECK_LAUNCH("splice_area_kernel");
    return 0;
}

int gsr_splice_edge_lengths(int n, int V, const long long* keys, const float* verts, double* length, int* err, gsr_stream_t stream)
{
    clear_error();
    if (n < 0 || V < 0) return fail_msg("gsr_splice_edge_lengths: negative size");
    if (n == 0) return 0;
    if (!keys || !length || !err || (V > 0 && !verts)) return fail_msg("gsr_splice_edge_lengths: required pointer is null");
    splice_edge_length_kernel<<<mesh_blocks(n), SP_BLOCK, 0, (hipStream_t)stream>>>(n, V, keys, verts, length, err);
    GSR_CHECK_LAUNCH("splice_edge_length_kernel");
    return 0;
}

int gsr_splice_mean(long long n, const double* x, void* workspace, double* mean, gsr_stream_t stream)
{
    clear_error();
    if (n <= 0) return fail_msg("gsr_splice_mean: n must be positive");
    if (!x || !workspace || !mean) return fail_msg("gsr_splice_mean: required pointer is null");
    if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(mean)) & 7)
        return fail_msg("gsr_splice_mean: arrays must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int n_wg = reduce_workgroups(n);
    double* partials = static_cast<double*>(workspace);
    splice_sum_kernel<<<(unsigned)n_wg, RED_BLOCK, 0, st>>>(n, x, partials);
    splice_mean_kernel<<<1, RED_BLOCK, 0, st>>>(n_wg, partials, n, mean);
    GSR_CHECK_LAUNCH("splice mean kernels");
    return 0;
}

}  // extern "C"
