// gsr_stitch.hip -- the stitch of update_mesh_topo's back half (gaustar_trainers/refined_mesh.py:463-693): connect_two_meshes
// (:158-215) with reset_duplicate_vert (:114-123) and merge_vert_around_holes (:126-155), the watertight test (:639) and the
// face-mask bookkeeping (:656-658).  fill_holes and the reference areas are in gsr_splice.hip; the chaining over boxes is
// gaustar_amd.regions.update_mesh_topology.
//
// The reference does this on the host with pytorch3d's knn_points, trimesh's group_rows / nondegenerate_faces /
// remove_unreferenced_vertices and scipy's connected_components.  Here, over device tensors:
//   nearest vertex      stitch_nn_kernel           the one O(Bq Bc) step: per query the (d2, index) minimum over the candidates,
//                                                  d2 in float64 without contraction; gsr_surface.h's tnn_search: 16 queries per
//                                                  workgroup, the candidates staged through LDS in tiles of 1024, split 16 ways
//   index lists         stitch_check_list_kernel   range and uniqueness of a boundary list, through the err word
//   snap groups         stitch_group_min / _remap_kernel   after the two snaps every listed vertex sits at an original pc1
//                                                  position, named by the LOWEST pc1 index that holds it (the nearest search
//                                                  breaks ties that way), so a group of equal positions is a group of equal
//                                                  source indices: its earliest list entry by integer atomicMin
//   degenerate faces    stitch_mark_kernel         faces rewritten by a vertex map, kept unless two indices are equal (or by a
//                                                  mask: select_faces); (two cumsums and gsr_regions_cut_emit compact)
//   holes               stitch_hole_edge_kernel    face-edges of count != 2 as vertex pairs; union-find over them
//                                                  (gsr_unionfind.h); stitch_hole_size / _move_kernel: components of at most
//                                                  max_hole_vert_num vertices collapse onto their lowest vertex
//   groups by position  stitch_pos_key / _head / _remap_kernel   (two stable torch.sorts of the coordinates' bits, a cummax)
//   bookkeeping         stitch_compose_mask / stitch_vert_map / stitch_watertight_kernel
// Every output is an integer or an exactly defined float.  No float atomics: the maximum of d2 is an integer atomicMax on the
// bits of the non-negative double, whose unsigned order is the doubles' order.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_internal.h"
#include "gsr_unionfind.h"
#include "gsr_surface.h"

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int ST_BLOCK = MESH_BLOCK;
constexpr int NN_TILE = 1024;       // candidates staged in LDS at once: 3 x 1024 doubles = 24 KiB

// idx [Bq], d2 [Bq]; max_bits [1] (zero before): the largest d2's bits.  grid = ceil(Bq / 16).  A coordinate that is not finite
// sets err bit 1 (the differences would be NaN and rank nothing); idx stays inside [0, Bc) even then.
__global__ void __launch_bounds__(TNN_BLOCK) stitch_nn_kernel(int Bq, int Bc, const float* __restrict__ q, const float* __restrict__ c,
                                                             int* __restrict__ idx, double* __restrict__ d2,
                                                             unsigned long long* __restrict__ max_bits, int* __restrict__ err)
{
    const int qi = blockIdx.x * TNN_QUERIES + tnn_query();
    const bool live = qi < Bq;
    double qx = 0., qy = 0., qz = 0.;
    if (live) {
        qx = (double)q[3 * (size_t)qi]; qy = (double)q[3 * (size_t)qi + 1]; qz = (double)q[3 * (size_t)qi + 2];
        if (tnn_owner() && !finite3(D3{qx, qy, qz})) atomicOr(err, MESH_ERR_NAN);
    }
    double bd;
    int bi;
    tnn_search<3, NN_TILE, 4>(
        Bc, bd, bi,
        [&](double (*tile)[NN_TILE], int base, int n) {
            const float* src = c + 3 * (size_t)base;
            for (int e = threadIdx.x; e < 3 * n; e += TNN_BLOCK) {
                const float v = src[e];
                if (blockIdx.x == 0 && (v - v) != 0.f) atomicOr(err, MESH_ERR_NAN);
                tile[e % 3][e / 3] = (double)v;
            }
        },
        [&](const double (*tile)[NN_TILE], int j) { return tnn_d2(tile, j, qx, qy, qz); });
    if (threadIdx.x >= 64) return;                           // (wave 0 holds the results; its 16 query lanes take the maximum)
    unsigned long long mb = 0ull;
    if (tnn_owner() && live) {
        idx[qi] = bi == TNN_NONE ? 0 : bi;
        d2[qi] = bd;
        if (bd == bd) mb = (unsigned long long)__double_as_longlong(bd);   // (bd >= 0: the bits' order is the values')
    }
#pragma unroll
    for (int m = 1; m < TNN_QUERIES; m <<= 1) {
        const unsigned long long o = __shfl_xor(mb, m);
        mb = o > mb ? o : mb;
    }
    if (threadIdx.x == 0 && mb) atomicMax(max_bits, mb);
}

// mark [V] int32 (zero before): err bit 0 for an index outside [0, V), bit 2 for an index listed twice
__global__ void __launch_bounds__(ST_BLOCK) stitch_check_list_kernel(int B, int V, const int* __restrict__ list, int* __restrict__ mark,
                                                                     int* __restrict__ err)
{
    const int i = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (i >= B) return;
    const int v = list[i];
    if ((unsigned)v >= (unsigned)V) { atomicOr(err, MESH_ERR_INDEX); return; }
    if (atomicAdd(mark + v, 1) != 0) atomicOr(err, MESH_ERR_DUP);
}

// ---------------------------------------------------------------------------------------------------- snap groups
// List entry p < B1 is vertex b1[p] and sits at pc1[n21[n12[p]]]; entry B1 + j is vertex V1 + b2[j] and sits at pc1[n21[j]].
__device__ __forceinline__ int snap_source(int p, int B1, const int* n21, const int* n12) { return p < B1 ? n21[n12[p]] : n21[p - B1]; }
__device__ __forceinline__ int snap_vertex(int p, int B1, int V1, const int* b1, const int* b2) { return p < B1 ? b1[p] : V1 + b2[p - B1]; }

__global__ void __launch_bounds__(ST_BLOCK) stitch_group_init_kernel(int B1, int V, int* __restrict__ rep, int* __restrict__ remap)
{
    const int i = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (i < B1) rep[i] = 0x7fffffff;
    if (i < V) remap[i] = i;
}

__global__ void __launch_bounds__(ST_BLOCK) stitch_group_min_kernel(int B1, int B2, const int* __restrict__ n21, const int* __restrict__ n12,
                                                                    int* __restrict__ rep)
{
    const int p = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (p < B1 + B2) atomicMin(rep + snap_source(p, B1, n21, n12), p);
}

__global__ void __launch_bounds__(ST_BLOCK) stitch_group_remap_kernel(int B1, int B2, int V1, const int* __restrict__ b1, const int* __restrict__ b2,
                                                                      const int* __restrict__ n21, const int* __restrict__ n12,
                                                                      const int* __restrict__ rep, int* __restrict__ remap)
{
    const int p = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (p >= B1 + B2) return;
    remap[snap_vertex(p, B1, V1, b1, b2)] = snap_vertex(rep[snap_source(p, B1, n21, n12)], B1, V1, b1, b2);
}

// ---------------------------------------------------------------------------------------------------- faces
// faces_rw [F,3] = remap[faces] (faces without a remap); keep [F] int32 = mask[f] with a mask, else all three indices differ
// (trimesh's nondegenerate_faces without its height test); ref [V] int32 (zero before) = the vertex belongs to a kept face.
__global__ void __launch_bounds__(ST_BLOCK) stitch_mark_kernel(int F, int V, const int* __restrict__ faces, const int* __restrict__ remap,
                                                               const unsigned char* __restrict__ mask, int* __restrict__ faces_rw,
                                                               int* __restrict__ keep, int* __restrict__ ref, int* __restrict__ err)
{
    const int f = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (f >= F) return;
    int v[3];
    if (!mesh_face(faces, f, V, v)) {
        atomicOr(err, MESH_ERR_INDEX);
        faces_rw[3 * (size_t)f] = 0; faces_rw[3 * (size_t)f + 1] = 0; faces_rw[3 * (size_t)f + 2] = 0;
        keep[f] = 0;
        return;
    }
    int a = v[0], b = v[1], c = v[2];
    if (remap) { a = remap[a]; b = remap[b]; c = remap[c]; }
    faces_rw[3 * (size_t)f] = a; faces_rw[3 * (size_t)f + 1] = b; faces_rw[3 * (size_t)f + 2] = c;
    const int kp = mask ? (mask[f] != 0) : (a != b && b != c && c != a);
    keep[f] = kp;
    if (kp) { ref[a] = 1; ref[b] = 1; ref[c] = 1; }
}

// ---------------------------------------------------------------------------------------------------- holes
// pairs [3 F]: the vertex pair of every face-edge whose count is not 2, (-1, -1) for the others; hole [V] uint8 (zero before)
__global__ void __launch_bounds__(ST_BLOCK) stitch_hole_edge_kernel(int F, int V, const int* __restrict__ faces, const int* __restrict__ counts,
                                                                    int2* __restrict__ pairs, unsigned char* __restrict__ hole,
                                                                    int* __restrict__ err)
{
    const int f = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (f >= F) return;
    int v[3];
    const bool ok = mesh_face(faces, f, V, v);
    if (!ok) atomicOr(err, MESH_ERR_INDEX);
    for (int e = 0; e < 3; ++e) {
        int2 pr = make_int2(-1, -1);
        if (ok && counts[3 * (size_t)f + e] != 2) {
            pr = make_int2(v[e], v[(e + 1) % 3]);
            hole[pr.x] = 1; hole[pr.y] = 1;
        }
        pairs[3 * (size_t)f + e] = pr;
    }
}

// size [V] (zero before): at a component's lowest vertex, its hole vertices
__global__ void __launch_bounds__(ST_BLOCK) stitch_hole_size_kernel(int V, const unsigned char* __restrict__ hole, const int* __restrict__ parent,
                                                                    int* __restrict__ size)
{
    const int v = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (v < V && hole[v]) atomicAdd(size + parent[v], 1);
}

// verts_out = verts, but a hole vertex of a component of at most max_n vertices takes its lowest vertex's position (:145-152)
__global__ void __launch_bounds__(ST_BLOCK) stitch_hole_move_kernel(int V, int max_n, const unsigned char* __restrict__ hole,
                                                                    const int* __restrict__ parent, const int* __restrict__ size,
                                                                    const float* __restrict__ verts, float* __restrict__ verts_out)
{
    const int v = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (v >= V) return;
    int s = v;
    if (hole[v] && size[parent[v]] <= max_n) s = parent[v];
    for (int a = 0; a < 3; ++a) verts_out[3 * (size_t)v + a] = verts[3 * (size_t)s + a];
}

// ---------------------------------------------------------------------------------------------------- groups by position
// Equal numbers have equal keys (-0 counts as +0); the keys' order means nothing, the sorts only bring equal ones together.
__global__ void __launch_bounds__(ST_BLOCK) stitch_pos_key_kernel(int H, const int* __restrict__ list, const float* __restrict__ verts,
                                                                  long long* __restrict__ key_xy, long long* __restrict__ key_z)
{
    const int i = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (i >= H) return;
    const float* p = verts + 3 * (size_t)list[i];
    const unsigned x = __float_as_uint(p[0] + 0.f), y = __float_as_uint(p[1] + 0.f), z = __float_as_uint(p[2] + 0.f);
    key_xy[i] = (long long)(((unsigned long long)x << 32) | y);
    key_z[i] = (long long)z;
}

// order [H] int64: the list entries sorted by (key_xy, key_z), equal ones in list order.  head [H] int32 = i where the entry
// at sorted position i differs in position from the one before it (a NaN differs from everything), 0 elsewhere: its
// running maximum is the first position of every run.
__global__ void __launch_bounds__(ST_BLOCK) stitch_pos_head_kernel(int H, const long long* __restrict__ order, const int* __restrict__ list,
                                                                   const float* __restrict__ verts, int* __restrict__ head)
{
    const int i = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (i >= H) return;
    int h = i;
    if (i > 0) {
        const float* p = verts + 3 * (size_t)list[order[i]];
        const float* o = verts + 3 * (size_t)list[order[i - 1]];
        if (p[0] == o[0] && p[1] == o[1] && p[2] == o[2]) h = 0;
    }
    head[i] = h;
}

// remap [V] (the identity before): every listed vertex -> the earliest listed vertex of its run
__global__ void __launch_bounds__(ST_BLOCK) stitch_pos_remap_kernel(int H, const long long* __restrict__ order, const int* __restrict__ list,
                                                                    const int* __restrict__ first, int* __restrict__ remap)
{
    const int i = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (i < H) remap[list[order[i]]] = list[order[first[i]]];
}

// ---------------------------------------------------------------------------------------------------- bookkeeping
// out [F] = outer[f] and inner[scan[f] - 1], scan the INCLUSIVE scan of outer: `m = outer; m[outer] = inner` (:205-206, :656-658)
__global__ void __launch_bounds__(ST_BLOCK) stitch_compose_mask_kernel(int F, const unsigned char* __restrict__ outer, const int* __restrict__ scan,
                                                                       const unsigned char* __restrict__ inner, int n_inner,
                                                                       unsigned char* __restrict__ out)
{
    const int f = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (f >= F) return;
    unsigned char o = 0;
    if (outer[f]) {
        const int k = scan[f] - 1;
        o = (k >= 0 && k < n_inner) ? (inner[k] != 0) : 0;
    }
    out[f] = o;
}

// out [V] = map2[remap2[map1[remap1[v]]]], -1 as soon as a map says dropped
__global__ void __launch_bounds__(ST_BLOCK) stitch_vert_map_kernel(int V, const int* __restrict__ remap1, const int* __restrict__ map1,
                                                                   const int* __restrict__ remap2, const int* __restrict__ map2,
                                                                   int* __restrict__ out)
{
    const int v = blockIdx.x * ST_BLOCK + threadIdx.x;
    if (v >= V) return;
    const int a = map1[remap1[v]];
    out[v] = a < 0 ? -1 : map2[remap2[a]];
}

// bad [1] (zero before) |= 1 where a face-edge's count is not 2
__global__ void __launch_bounds__(ST_BLOCK) stitch_watertight_kernel(long long n, const int* __restrict__ counts, int* __restrict__ bad)
{
    const long long i = (long long)blockIdx.x * ST_BLOCK + threadIdx.x;
    const bool b = i < n && counts[i] != 2;
    if (__ballot(b) && (threadIdx.x & 63) == 0) atomicOr(bad, 1);
}

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

int gsr_stitch_nn_tile(void) { return NN_TILE; }
int gsr_stitch_nn_queries(void) { return TNN_QUERIES; }

int gsr_stitch_nearest(int Bq, int Bc, const float* queries, const float* candidates, int* idx, double* d2,
                       unsigned long long* max_bits, int* err, gsr_stream_t stream)
{
    clear_error();
    if (Bq < 0 || Bc < 0) return fail_msg("gsr_stitch_nearest: negative size");
    if (!max_bits) return fail_msg("gsr_stitch_nearest: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    GSR_CHECK(hipMemsetAsync(max_bits, 0, sizeof(unsigned long long), st));
    if (Bq == 0) return 0;
    if (Bc == 0) return fail_msg("gsr_stitch_nearest: no candidates");
    if (!queries || !candidates || !idx || !d2 || !err) return fail_msg("gsr_stitch_nearest: required pointer is null");
    stitch_nn_kernel<<<(unsigned)((Bq + TNN_QUERIES - 1) / TNN_QUERIES), TNN_BLOCK, 0, st>>>(Bq, Bc, queries, candidates, idx, d2, max_bits, err);
    GSR_CHECK_LAUNCH("stitch_nn_kernel");
    return 0;
}

int gsr_stitch_check_list(int B, int V, const int* list, int* mark, int* err, gsr_stream_t stream)
{
    clear_error();
    if (B < 0 || V < 0) return fail_msg("gsr_stitch_check_list: negative size");
    if (B == 0) return 0;
    if (!list || !err || (V > 0 && !mark)) return fail_msg("gsr_stitch_check_list: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    if (V > 0) GSR_CHECK(hipMemsetAsync(mark, 0, sizeof(int) * (size_t)V, st));
    stitch_check_list_kernel<<<mesh_blocks(B), ST_BLOCK, 0, st>>>(B, V, list, mark, err);
    GSR_CHECK_LAUNCH("stitch_check_list_kernel");
    return 0;
}

int gsr_stitch_snap_groups(int B1, int B2, int V1, int V2, const int* b1, const int* b2, const int* n21, const int* n12, int* rep,
                           int* remap, gsr_stream_t stream)
{
    clear_error();
    if (B1 <= 0 || B2 <= 0 || V1 <= 0 || V2 <= 0 || (long long)V1 + V2 > 0x7fffffff || (long long)B1 + B2 > 0x7fffffff)
        return fail_msg("gsr_stitch_snap_groups: sizes must be positive and their sums below 2^31");
    if (!b1 || !b2 || !n21 || !n12 || !rep || !remap) return fail_msg("gsr_stitch_snap_groups: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    const int V = V1 + V2, B = B1 + B2;
    stitch_group_init_kernel<<<mesh_blocks(V > B1 ? V : B1), ST_BLOCK, 0, st>>>(B1, V, rep, remap);
    stitch_group_min_kernel<<<mesh_blocks(B), ST_BLOCK, 0, st>>>(B1, B2, n21, n12, rep);
    stitch_group_remap_kernel<<<mesh_blocks(B), ST_BLOCK, 0, st>>>(B1, B2, V1, b1, b2, n21, n12, rep, remap);
    GSR_CHECK_LAUNCH("stitch snap-group kernels");
    return 0;
}

int gsr_stitch_mark(int F, int V, const int* faces, const int* remap, const unsigned char* mask, int* faces_out, int* keep,
                    int* referenced, int* err, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || V < 0) return fail_msg("gsr_stitch_mark: negative size or too many faces");
    if ((V > 0 && !referenced) || (F > 0 && (!faces || !faces_out || !keep || !err)))
        return fail_msg("gsr_stitch_mark: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    if (V > 0) GSR_CHECK(hipMemsetAsync(referenced, 0, sizeof(int) * (size_t)V, st));
    if (F > 0) stitch_mark_kernel<<<mesh_blocks(F), ST_BLOCK, 0, st>>>(F, V, faces, remap, mask, faces_out, keep, referenced, err);
    GSR_CHECK_LAUNCH("stitch_mark_kernel");
    return 0;
}

int gsr_stitch_hole_components(int F, int V, const int* faces, const int* counts, int* pairs, unsigned char* hole, int* parent,
                               int* root_flag, int* err, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || V < 0) return fail_msg("gsr_stitch_hole_components: negative size or too many faces");
    if (V == 0) return 0;
    if (!hole || !parent || !root_flag || (F > 0 && (!faces || !counts || !pairs || !err)))
        return fail_msg("gsr_stitch_hole_components: required pointer is null");
    if (reinterpret_cast<uintptr_t>(pairs) & 7) return fail_msg("gsr_stitch_hole_components: pairs must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    GSR_CHECK(hipMemsetAsync(hole, 0, (size_t)V, st));
    if (F > 0) stitch_hole_edge_kernel<<<mesh_blocks(F), ST_BLOCK, 0, st>>>(F, V, faces, counts, reinterpret_cast<int2*>(pairs), hole, err);
    launch_union_find(V, 3ll * F, reinterpret_cast<const int2*>(pairs), hole, parent, root_flag, st);
    GSR_CHECK_LAUNCH("stitch hole-component kernels");
    return 0;
}

int gsr_stitch_hole_move(int V, int max_hole_vert_num, const unsigned char* hole, const int* parent, int* size, const float* verts,
                         float* verts_out, gsr_stream_t stream)
{
    clear_error();
    if (V < 0) return fail_msg("gsr_stitch_hole_move: negative size");
    if (V == 0) return 0;
    if (!hole || !parent || !size || !verts || !verts_out) return fail_msg("gsr_stitch_hole_move: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    GSR_CHECK(hipMemsetAsync(size, 0, sizeof(int) * (size_t)V, st));
    stitch_hole_size_kernel<<<mesh_blocks(V), ST_BLOCK, 0, st>>>(V, hole, parent, size);
    stitch_hole_move_kernel<<<mesh_blocks(V), ST_BLOCK, 0, st>>>(V, max_hole_vert_num, hole, parent, size, verts, verts_out);
    GSR_CHECK_LAUNCH("stitch hole-move kernels");
    return 0;
}

int gsr_stitch_pos_keys(int H, const int* list, const float* verts, long long* key_xy, long long* key_z, gsr_stream_t stream)
{
    clear_error();
    if (H < 0) return fail_msg("gsr_stitch_pos_keys: negative size");
    if (H == 0) return 0;
    if (!list || !verts || !key_xy || !key_z) return fail_msg("gsr_stitch_pos_keys: required pointer is null");
    stitch_pos_key_kernel<<<mesh_blocks(H), ST_BLOCK, 0, (hipStream_t)stream>>>(H, list, verts, key_xy, key_z);
    GSR_CHECK_LAUNCH("stitch_pos_key_kernel");
    return 0;
}

int gsr_stitch_pos_heads(int H, const long long* order, const int* list, const float* verts, int* head, gsr_stream_t stream)
{
    clear_error();
    if (H < 0) return fail_msg("gsr_stitch_pos_heads: negative size");
    if (H == 0) return 0;
    if (!order || !list || !verts || !head) return fail_msg("gsr_stitch_pos_heads: required pointer is null");
    stitch_pos_head_kernel<<<mesh_blocks(H), ST_BLOCK, 0, (hipStream_t)stream>>>(H, order, list, verts, head);
    GSR_CHECK_LAUNCH("stitch_pos_head_kernel");
    return 0;
}

int gsr_stitch_pos_remap(int H, const long long* order, const int* list, const int* first, int* remap, gsr_stream_t stream)
{
    clear_error();
    if (H < 0) return fail_msg("gsr_stitch_pos_remap: negative size");
    if (H == 0) return 0;
    if (!order || !list || !first || !remap) return fail_msg("gsr_stitch_pos_remap: required pointer is null");
    stitch_pos_remap_kernel<<<mesh_blocks(H), ST_BLOCK, 0, (hipStream_t)stream>>>(H, order, list, first, remap);
    GSR_CHECK_LAUNCH("stitch_pos_remap_kernel");
    return 0;
}

int gsr_stitch_compose_mask(int F, const unsigned char* outer, const int* outer_scan, const unsigned char* inner, int n_inner,
                            unsigned char* out, gsr_stream_t stream)
{
    clear_error();
    if (F < 0 || n_inner < 0) return fail_msg("gsr_stitch_compose_mask: negative size");
    if (F == 0) return 0;
    if (!outer || !outer_scan || !out || (n_inner > 0 && !inner)) return fail_msg("gsr_stitch_compose_mask: required pointer is null");
    stitch_compose_mask_kernel<<<mesh_blocks(F), ST_BLOCK, 0, (hipStream_t)stream>>>(F, outer, outer_scan, inner, n_inner, out);
    GSR_CHECK_LAUNCH("stitch_compose_mask_kernel");
    return 0;
}

int gsr_stitch_vert_map(int V, const int* remap1, const int* map1, const int* remap2, const int* map2, int* out, gsr_stream_t stream)
{
    clear_error();
    if (V < 0) return fail_msg("gsr_stitch_vert_map: negative size");
    if (V == 0) return 0;
    if (!remap1 || !map1 || !remap2 || !map2 || !out) return fail_msg("gsr_stitch_vert_map: required pointer is null");
    stitch_vert_map_kernel<<<mesh_blocks(V), ST_BLOCK, 0, (hipStream_t)stream>>>(V, remap1, map1, remap2, map2, out);
    GSR_CHECK_LAUNCH("stitch_vert_map_kernel");
    return 0;
}

int gsr_stitch_watertight(int F, const int* counts, int* bad, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F)) return fail_msg("gsr_stitch_watertight: F must be in [0, (2^31 - 1) / 3]");
    if (!bad) return fail_msg("gsr_stitch_watertight: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    GSR_CHECK(hipMemsetAsync(bad, 0, sizeof(int), st));
    if (F == 0) return 0;
    if (!counts) return fail_msg("gsr_stitch_watertight: required pointer is null");
    stitch_watertight_kernel<<<mesh_blocks(3ll * F), ST_BLOCK, 0, st>>>(3ll * F, counts, bad);
    GSR_CHECK_LAUNCH("stitch_watertight_kernel");
    return 0;
}

}  // extern "C"
