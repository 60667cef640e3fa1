// gsr_topo.hip -- rig-wide topology-error detection (gaustar_trainers/refined_mesh.py:697-920, `detect_topo_err`, depth term):
// where the refined mesh disagrees with the GT depth of the rig, as a per-face weight that decides loose binding
// (refine.py:720-734).
//
// The reference runs it on the host: per camera a cv2.blur edge map (gaustar_tools/warp_mesh.py:120-130), a projection and
// three lookups per vertex (:57-74, :106-117); over the rig a Python mean per vertex, up to 20 Python propagation sweeps
// (mesh_vert_propagate, :133-155), an open3d voxel grid (:185-197) and a pytorch3d kNN interpolation (:199-213), then trimesh's
// vertex-to-face colour.  Here:
//   per camera  (3 launches, no host round trip; the camera, the edge statistic and the two image passes are gsr_rig.h's)
//     topo_gt_max_kernel    per-workgroup max of the GT depth below max_depth            -> partials[0, RIG_PARTS)
//     topo_var_max_kernel   per-workgroup max of the 3x3 edge statistic `var`            -> partials[RIG_PARTS, 2 RIG_PARTS)
//     topo_view_kernel      one lane per vertex: f64 projection, lookup, visibility, loss -> one row of the [C, V] table
//   over the rig
//     topo_aggregate_kernel  count, f64 mean in camera order, depth scalar, floor          (refined_mesh.py:826-891)
//     topo_propagate_kernel  one Jacobi sweep over a CSR neighbour list (ping-pong)        (mesh_vert_propagate)
//     topo_voxel_key_kernel / topo_voxel_reduce_kernel  open3d's voxel index, the ordered per-voxel mean and centre
//     topo_knn_bound / _part / _merge_kernel  exact K = 8 nearest voxel centres (a bound from the own voxel's neighbourhood,
//                            brute force over TP_SPLIT voxel ranges tiled through LDS, a merge), weighted f64 mean
//     topo_face_kernel       int(min(255 v, 255)) per vertex, mean of three truncated to uint8 per face, / 255
// No float atomics anywhere: every output is a pure function of the inputs (bitwise reproducible, independent of how many
// views are in flight and of how the cameras were sharded over ranks).
//
// Floating point follows the numpy restatement in tests/topo_ref.py operation by operation, so contraction into FMAs is off
// for this file: a fused multiply-add rounds once where numpy rounds twice.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_rig.h"

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int TP_BLOCK = RIG_BLOCK;   // the rig-wide kernels and the kNN tile; the per-camera kernels must run RIG_BLOCK lanes
constexpr int TP_SEED = 16;     // kNN bound: voxels on either side of a vertex's own voxel (sort order)
constexpr int TP_SPLIT = 8;     // kNN: voxel ranges scanned by separate workgroups
constexpr int TP_K = 8;         // interpolate_in_voxel(knn_K=8)

__global__ void __launch_bounds__(RIG_BLOCK) topo_gt_max_kernel(int n, const float* __restrict__ gt, float max_depth,
                                                                float* __restrict__ parts)
{
    depth_max_pass(n, gt, max_depth, 0, parts);
}

// get_depth_edge(depth_gt, 3): the 3x3 window
__global__ void __launch_bounds__(RIG_BLOCK) topo_var_max_kernel(int H, int W, const float* __restrict__ gt, float* __restrict__ parts)
{
    var_max_pass<1>(H, W, gt, 0, 1, parts);
}

__global__ void __launch_bounds__(RIG_BLOCK) topo_view_kernel(int H, int W, int V, const float* __restrict__ verts,
                                                              const float* __restrict__ gt, const float* __restrict__ render,
                                                              const float* __restrict__ surface, float max_depth,
                                                              const float* __restrict__ parts, RigCamera cam, float* __restrict__ row)
{
    __shared__ float red[RIG_BLOCK];
    const float gmax = block_max_of_parts(parts, red);
    const float vmax = block_max_of_parts(parts + RIG_PARTS, red);
    const int v = blockIdx.x * RIG_BLOCK + threadIdx.x;
    if (v >= V) return;
    // a camera without GT below max_depth (the reference raises on the empty max) or with a flat GT (max(var) = 0: edge_vis
    // is NaN and nothing passes `< 0.1`) sees no vertex
    if (gmax == -INFINITY || !(vmax > 0.f)) { row[v] = -1.f; return; }
    const float m = clip_depth(gmax);
    double lx, ly, lz, pr, pc;
    rig_project(cam, H, W, verts[3 * v], verts[3 * v + 1], verts[3 * v + 2], lx, ly, lz, pr, pc);
    bool ok = true;
    const int iy = rig_query(pr, H, ok), ix = rig_query(pc, W, ok);
    if (!ok) { row[v] = -1.f; return; }
    const size_t p = (size_t)iy * W + ix;
    const float s = surface[p];
    const float ev = fminf(__fdiv_rn(edge_var<1>(gt, H, W, iy, ix, m), vmax) * 1000.f, 1.f);   // refined_mesh.py:792
    if (!(fabs(lz - (double)s) < 0.005) || !(ev < 0.1f)) { row[v] = -1.f; return; }          // :790-794
    row[v] = fminf(fabsf(fminf(gt[p], max_depth) - render[p]) * (1.f - ev) * 10.f, 2.f);     // :780, :799
}

__global__ void __launch_bounds__(TP_BLOCK) topo_aggregate_kernel(int C, int V, const float* __restrict__ table,
                                                                  const float* __restrict__ verts, const float* __restrict__ ymin,
                                                                  double depth_scalar, int min_observe, int detect_floor,
                                                                  double* __restrict__ value, int* __restrict__ cnt_out,
                                                                  unsigned char* __restrict__ valid)
{
    const int v = blockIdx.x * TP_BLOCK + threadIdx.x;
    if (v >= V) return;
    int cnt = 0;
    double sum = 0.0;
    for (int c = 0; c < C; ++c) {
        const float x = table[(size_t)c * V + v];
        if (x != -1.f) { sum += (double)x; ++cnt; }   // (-1 = not visible; a recorded NaN stays a NaN, as in the reference)
    }
    double val = cnt >= min_observe ? sum / cnt : 0.0;   // refined_mesh.py:826-837
    val = val * depth_scalar;                            // :845
    if (detect_floor && (double)verts[3 * v + 1] < (double)ymin[0] + 0.02) {   // :869-875
        val = 0.0;
        cnt = min_observe + 1;
    }
    value[v] = val;
    cnt_out[v] = cnt;
    valid[v] = cnt >= min_observe;
}

// one sweep of mesh_vert_propagate: the reference's loop writes in place but reads only vertices that were valid before the
// sweep, which is this Jacobi step
__global__ void __launch_bounds__(TP_BLOCK) topo_propagate_kernel(int V, const int* __restrict__ off, const int* __restrict__ nbr,
                                                                  const double* __restrict__ vin, const unsigned char* __restrict__ okin,
                                                                  double* __restrict__ vout, unsigned char* __restrict__ okout)
{
    const int v = blockIdx.x * TP_BLOCK + threadIdx.x;
    if (v >= V) return;
    double val = vin[v];
    unsigned char ok = okin[v];
    if (!ok) {
        double s = 0.0;
        int k = 0;
        for (int e = off[v]; e < off[v + 1]; ++e) {
            const int u = nbr[e];
            if (okin[u]) { s += vin[u]; ++k; }
        }
        if (k) { val = s / k; ok = 1; }
    }
    vout[v] = val;
    okout[v] = ok;
}

constexpr int VX_BITS = 21;   // voxel index bits per axis in the sort key

// open3d VoxelGrid::CreateFromPointCloud: origin = min_bound - voxel_size / 2, index = floor((v - origin) / voxel_size)
__global__ void __launch_bounds__(TP_BLOCK) topo_voxel_key_kernel(int V, const float* __restrict__ verts, const float* __restrict__ vmin,
                                                                  double voxel_size, long long* __restrict__ keys, int* __restrict__ flags)
{
    const int v = blockIdx.x * TP_BLOCK + threadIdx.x;
    if (v >= V) return;
    long long key = 0;
    for (int a = 0; a < 3; ++a) {
        const double origin = (double)vmin[a] - voxel_size * 0.5;
        const double f = floor(((double)verts[3 * v + a] - origin) / voxel_size);
        if (!(f >= 0.0 && f < (double)(1 << VX_BITS))) { flags[0] = 1; key = 0; break; }   // (checked by the caller)
        key = (key << VX_BITS) | (long long)f;
    }
    keys[v] = key;
}

// per voxel (a run of equal keys in the stably sorted order, i.e. its vertices in index order, as open3d adds them): the mean
// of the values and the centre origin + (index + 0.5) voxel_size
__global__ void __launch_bounds__(TP_BLOCK) topo_voxel_reduce_kernel(int V, const long long* __restrict__ skeys,
                                                                     const long long* __restrict__ perm, const long long* __restrict__ vid,
                                                                     const double* __restrict__ value, const float* __restrict__ vmin,
                                                                     double voxel_size, float4* __restrict__ centre,
                                                                     double* __restrict__ vox_value, int* __restrict__ own)
{
    const int i = blockIdx.x * TP_BLOCK + threadIdx.x;
    if (i >= V) return;
    const long long key = skeys[i];
    own[perm[i]] = (int)vid[i];
    if (i > 0 && skeys[i - 1] == key) return;
    double s = 0.0;
    int n = 0;
    for (int j = i; j < V && skeys[j] == key; ++j) { s += value[perm[j]]; ++n; }
    const long long id = vid[i];
    vox_value[id] = s / n;
    const long long mask = (1ll << VX_BITS) - 1;
    const long long idx[3] = {key >> (2 * VX_BITS), (key >> VX_BITS) & mask, key & mask};
    float c[3];
    for (int a = 0; a < 3; ++a) c[a] = (float)(((double)vmin[a] - voxel_size * 0.5) + ((double)idx[a] + 0.5) * voxel_size);
    centre[id] = make_float4(c[0], c[1], c[2], 0.f);
}

// interpolate_in_voxel: the K = 8 nearest voxel centres by f32 squared distance ((dx^2 + dy^2) + dz^2, pytorch3d's
// knn_points), ties to the lower voxel index; weights exp(-d^2 / voxel_size^2) + 1e-8 and the weighted mean in f64.  Slots
// beyond the number of voxels are index 0 at distance 0, as knn_points leaves them.  Exact brute force in three launches:
//   bound  per vertex: the 8 nearest among the 2 TP_SEED + 1 voxels around its own voxel in sort order (its x slab, nearby y
//          rows); their 8th distance tau bounds the true 8th distance from above;
//   part   (vertex block, split): one of TP_SPLIT consecutive ranges of voxels, streamed through LDS in tiles of TP_BLOCK,
//          candidates with d <= tau kept as a top 8 -- TP_SPLIT times the workgroups of one pass over all voxels, which
//          at config C (161 vertex blocks) leaves most SIMDs idle;
//   merge  per vertex: the TP_SPLIT lists into one top 8, then the weighted mean.
// Top-8 lists are ordered by (distance, index), so the result does not depend on the order candidates arrive in.
__device__ __forceinline__ void knn_offer(float d, int id, float (&bd)[TP_K], int (&bi)[TP_K])
{
    if (d < bd[TP_K - 1] || (d == bd[TP_K - 1] && id < bi[TP_K - 1])) {
#pragma unroll
        for (int k = 0; k < TP_K; ++k) {
            if (d < bd[k] || (d == bd[k] && id < bi[k])) {
                const float td = bd[k]; const int ti = bi[k];
                bd[k] = d; bi[k] = id; d = td; id = ti;
            }
        }
    }
}

__device__ __forceinline__ float knn_dist(float qx, float qy, float qz, float4 c)
{
    const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
    return dx * dx + dy * dy + dz * dz;
}

__device__ __forceinline__ void knn_init(float (&bd)[TP_K], int (&bi)[TP_K])
{
#pragma unroll
    for (int k = 0; k < TP_K; ++k) { bd[k] = INFINITY; bi[k] = 0x7fffffff; }
}

__global__ void __launch_bounds__(TP_BLOCK) topo_knn_bound_kernel(int V, const float* __restrict__ verts, const float4* __restrict__ centre,
                                                                  const long long* __restrict__ last_vid, const int* __restrict__ own,
                                                                  float* __restrict__ tau)
{
    const int v = blockIdx.x * TP_BLOCK + threadIdx.x;
    if (v >= V) return;
    const int nvox = (int)last_vid[0] + 1;
    const float qx = verts[3 * v], qy = verts[3 * v + 1], qz = verts[3 * v + 2];
    float bd[TP_K];
    int bi[TP_K];
    knn_init(bd, bi);
    const int lo = max(0, own[v] - TP_SEED), hi = min(nvox, own[v] + TP_SEED + 1);
    for (int id = lo; id < hi; ++id) knn_offer(knn_dist(qx, qy, qz, centre[id]), id, bd, bi);
    tau[v] = bd[TP_K - 1];   // (inf with fewer than 8 voxels in the window: no bound)
}

__global__ void __launch_bounds__(TP_BLOCK) topo_knn_part_kernel(int V, const float* __restrict__ verts, const float4* __restrict__ centre,
                                                                 const long long* __restrict__ last_vid, const float* __restrict__ tau,
                                                                 float* __restrict__ part_d, int* __restrict__ part_i)
{
    __shared__ float4 tile[TP_BLOCK];
    const int nvox = (int)last_vid[0] + 1;
    const int chunk = (nvox + TP_SPLIT - 1) / TP_SPLIT;
    const int begin = blockIdx.y * chunk, end = min(nvox, begin + chunk);
    const int v = blockIdx.x * TP_BLOCK + threadIdx.x;
    const bool live = v < V;
    const float qx = live ? verts[3 * v] : 0.f, qy = live ? verts[3 * v + 1] : 0.f, qz = live ? verts[3 * v + 2] : 0.f;
    const float t = live ? tau[v] : -1.f;
    float bd[TP_K];
    int bi[TP_K];
    knn_init(bd, bi);
    for (int base = begin; base < end; base += TP_BLOCK) {
        __syncthreads();
        if (base + (int)threadIdx.x < end) tile[threadIdx.x] = centre[base + threadIdx.x];
        __syncthreads();
        const int n = min(TP_BLOCK, end - base);
        for (int j = 0; j < n; ++j) {
            const float d = knn_dist(qx, qy, qz, tile[j]);
            if (d <= t) knn_offer(d, base + j, bd, bi);
        }
    }
    if (!live) return;
    const size_t o = ((size_t)blockIdx.y * V + v) * TP_K;
#pragma unroll
    for (int k = 0; k < TP_K; ++k) { part_d[o + k] = bd[k]; part_i[o + k] = bi[k]; }
}

__global__ void __launch_bounds__(TP_BLOCK) topo_knn_merge_kernel(int V, const float* __restrict__ part_d, const int* __restrict__ part_i,
                                                                  const double* __restrict__ vox_value, double vs2, double* __restrict__ out)
{
    const int v = blockIdx.x * TP_BLOCK + threadIdx.x;
    if (v >= V) return;
    float bd[TP_K];
    int bi[TP_K];
    knn_init(bd, bi);
    for (int s = 0; s < TP_SPLIT; ++s) {
        const size_t o = ((size_t)s * V + v) * TP_K;
        for (int k = 0; k < TP_K; ++k) {
            const float d = part_d[o + k];
            if (d == INFINITY) break;
            knn_offer(d, part_i[o + k], bd, bi);
        }
    }
    double sw = 0.0, swv = 0.0;
#pragma unroll
    for (int k = 0; k < TP_K; ++k) {
        const bool have = bd[k] != INFINITY;
        const double w = exp(-(double)(have ? bd[k] : 0.f) / vs2) + 1e-8;
        swv += vox_value[have ? bi[k] : 0] * w;
        sw += w;
    }
    out[v] = swv / sw;
}

// trimesh: vertex colour int(min(255 v, 255)) (refined_mesh.py:913-914), face colour = mean of its three vertex colours cast
// to uint8, which truncates; face_loss = face colour / 255 (:915, :920)
__device__ __forceinline__ int vertex_colour(double v)
{
    const double c = fmin(v * 255.0, 255.0);
    return c >= 0.0 ? (int)c : 0;   // (values are >= 0; NaN reads as 0, as NumPy's cast to uint8 of INT_MIN)
}

__global__ void __launch_bounds__(TP_BLOCK) topo_face_kernel(int F, const int* __restrict__ faces, const double* __restrict__ value,
                                                             unsigned char* __restrict__ colour, float* __restrict__ loss)
{
    const int f = blockIdx.x * TP_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int c = (vertex_colour(value[faces[3 * f]]) + vertex_colour(value[faces[3 * f + 1]]) + vertex_colour(value[faces[3 * f + 2]])) / 3;
    colour[f] = (unsigned char)c;
    loss[f] = (float)((double)c / 255.0);
}

inline int blocks(int n) { return (n + TP_BLOCK - 1) / TP_BLOCK; }

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

size_t gsr_topo_view_workspace_bytes(int H, int W)
{
    (void)H; (void)W;   // (the partial maxima of a fixed number of workgroups, whatever the image)
    return 2 * RIG_PARTS * sizeof(float);
}

int gsr_topo_view(int H, int W, int V, const float* verts, const float* depth_gt, const float* render_depth,
                  const float* surface_depth, float max_depth, const double* cam, void* workspace, float* row, gsr_stream_t stream)
{
    clear_error();
    if (H <= 0 || W <= 0 || V < 0) return fail_msg("gsr_topo_view: sizes must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail_msg("gsr_topo_view: image too large");
    if (!depth_gt || !render_depth || !surface_depth || !cam || !workspace || (V > 0 && (!verts || !row)))
        return fail_msg("gsr_topo_view: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    float* parts = static_cast<float*>(workspace);
    topo_gt_max_kernel<<<RIG_PARTS, RIG_BLOCK, 0, st>>>(H * W, depth_gt, max_depth, parts);
    topo_var_max_kernel<<<RIG_PARTS, RIG_BLOCK, 0, st>>>(H, W, depth_gt, parts);
    if (V > 0)
        topo_view_kernel<<<blocks(V), RIG_BLOCK, 0, st>>>(H, W, V, verts, depth_gt, render_depth, surface_depth, max_depth, parts,
                                                          rig_camera(cam), row);
    GSR_CHECK_LAUNCH("topo view kernels");
    return 0;
}

int gsr_topo_aggregate(int C, int V, const float* table, const float* verts, const float* ymin, double depth_scalar,
                       int min_observe, int detect_floor, double* value, int* count, unsigned char* valid, gsr_stream_t stream)
{
    clear_error();
    if (C < 0 || V < 0) return fail_msg("gsr_topo_aggregate: negative size");
    if (V == 0) return 0;
    if ((C > 0 && !table) || !verts || !value || !count || !valid || (detect_floor && !ymin))
        return fail_msg("gsr_topo_aggregate: required pointer is null");
    topo_aggregate_kernel<<<blocks(V), TP_BLOCK, 0, (hipStream_t)stream>>>(C, V, table, verts, ymin, depth_scalar, min_observe,
                                                                           detect_floor != 0, value, count, valid);
    GSR_CHECK_LAUNCH("topo_aggregate_kernel");
    return 0;
}

int gsr_topo_propagate(int V, const int* nbr_offsets, const int* nbr, int sweeps, const double* value_in,
                       const unsigned char* valid_in, double* value_out, double* value_tmp, unsigned char* valid_a,
                       unsigned char* valid_b, gsr_stream_t stream)
{
    clear_error();
    if (V < 0 || sweeps < 0) return fail_msg("gsr_topo_propagate: negative size");
    if (V == 0) return 0;
    if (!value_in || !value_out) return fail_msg("gsr_topo_propagate: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    if (sweeps == 0) {
        GSR_CHECK(hipMemcpyAsync(value_out, value_in, sizeof(double) * V, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    if (!nbr_offsets || !nbr || !valid_in || !value_tmp || !valid_a || !valid_b)
        return fail_msg("gsr_topo_propagate: required pointer is null");
    unsigned char* ob[2] = {valid_a, valid_b};
    const unsigned char* osrc = valid_in;
    ping_pong_sweeps(sweeps, value_in, value_out, value_tmp, [&](const double* src, double* dst, int k) {
        topo_propagate_kernel<<<blocks(V), TP_BLOCK, 0, st>>>(V, nbr_offsets, nbr, src, osrc, dst, ob[k]);
        osrc = ob[k];
    });
    GSR_CHECK_LAUNCH("topo_propagate_kernel");
    return 0;
}

int gsr_topo_voxel_keys(int V, const float* verts, const float* vmin, double voxel_size, long long* keys, int* flags,
                        gsr_stream_t stream)
{
    clear_error();
    if (V < 0) return fail_msg("gsr_topo_voxel_keys: negative size");
    if (!(voxel_size > 0.0)) return fail_msg("gsr_topo_voxel_keys: voxel_size must be positive");
    if (V == 0) return 0;
    if (!verts || !vmin || !keys || !flags) return fail_msg("gsr_topo_voxel_keys: required pointer is null");
    topo_voxel_key_kernel<<<blocks(V), TP_BLOCK, 0, (hipStream_t)stream>>>(V, verts, vmin, voxel_size, keys, flags);
    GSR_CHECK_LAUNCH("topo_voxel_key_kernel");
    return 0;
}

size_t gsr_topo_voxel_workspace_bytes(int V)
{
    // centres [V] float4, own voxel [V] int, tau [V] float, TP_SPLIT partial top-8 lists of (float, int)
    return V > 0 ? (size_t)V * (16 + 4 + 4 + (size_t)TP_SPLIT * TP_K * 8) : 0;
}

int gsr_topo_voxel_interp(int V, const float* verts, const float* vmin, double voxel_size, const long long* sorted_keys,
                          const long long* order, const long long* voxel_id, const double* value, void* workspace,
                          double* voxel_value, double* out, gsr_stream_t stream)
{
    clear_error();
    if (V < 0) return fail_msg("gsr_topo_voxel_interp: negative size");
    if (!(voxel_size > 0.0)) return fail_msg("gsr_topo_voxel_interp: voxel_size must be positive");
    if (V == 0) return 0;
    if (!verts || !vmin || !sorted_keys || !order || !voxel_id || !value || !workspace || !voxel_value || !out)
        return fail_msg("gsr_topo_voxel_interp: required pointer is null");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail_msg("gsr_topo_voxel_interp: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    float4* c4 = static_cast<float4*>(workspace);
    int* own = reinterpret_cast<int*>(c4 + V);
    float* tau = reinterpret_cast<float*>(own + V);
    float* part_d = tau + V;
    int* part_i = reinterpret_cast<int*>(part_d + (size_t)TP_SPLIT * TP_K * V);
    const long long* last = voxel_id + (V - 1);
    topo_voxel_reduce_kernel<<<blocks(V), TP_BLOCK, 0, st>>>(V, sorted_keys, order, voxel_id, value, vmin, voxel_size, c4, voxel_value, own);
    topo_knn_bound_kernel<<<blocks(V), TP_BLOCK, 0, st>>>(V, verts, c4, last, own, tau);
    topo_knn_part_kernel<<<dim3(blocks(V), TP_SPLIT), TP_BLOCK, 0, st>>>(V, verts, c4, last, tau, part_d, part_i);
    topo_knn_merge_kernel<<<blocks(V), TP_BLOCK, 0, st>>>(V, part_d, part_i, voxel_value, voxel_size * voxel_size, out);
    GSR_CHECK_LAUNCH("topo voxel kernels");
    return 0;
}

int gsr_topo_faces(int F, const int* faces, const double* value, unsigned char* face_colour, float* face_loss,
                   gsr_stream_t stream)
{
    clear_error();
    if (F < 0) return fail_msg("gsr_topo_faces: negative size");
    if (F == 0) return 0;
    if (!faces || !value || !face_colour || !face_loss) return fail_msg("gsr_topo_faces: required pointer is null");
    topo_face_kernel<<<blocks(F), TP_BLOCK, 0, (hipStream_t)stream>>>(F, faces, value, face_colour, face_loss);
    GSR_CHECK_LAUNCH("topo_face_kernel");
    return 0;
}

}  // extern "C"
