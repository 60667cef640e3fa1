// gsr_warp.hip -- scene-flow mesh warping to the next frame (gaustar_tools/warp_mesh.py:216-401, `warp_mesh_using_flow`
// with post_processing = 'mesh'): the refined mesh of frame f, moved along the optical flow of every camera onto the depth of
// frame f + interval, is the mesh frame f + interval starts from (train_seq.py:112, :242-245).
//
// The reference runs it on the host in numpy with trimesh and cv2: per camera two 7x7 edge maps, a pad / resize of the two
// RAFT flows, a projection and seven lookups per vertex (:259-340); over the rig a Python loop per vertex with outlier removal
// (:347-358), up to 20 propagation sweeps (:384, :133-155) and 5 smoothing sweeps (:394, :158-171).  Here:
//   once per warp
//     warp_face_kernel / warp_vertex_normal_kernel  trimesh Trimesh.vertex_normals in world space (rotated per camera)
//   per camera  (3 launches, no host round trip; the camera, the edge statistic and the two image passes are gsr_rig.h's)
//     warp_depth_max_kernel  per-workgroup max of depth_cur / depth_next below 10          -> partials [0, 2 RIG_PARTS)
//     warp_var_max_kernel    per-workgroup max of the 7x7 edge statistic of both maps       -> partials [2, 4 RIG_PARTS)
//     warp_view_kernel       one lane per vertex, :286-340 in f64                           -> one row [V,3] of the [C,V,3] table
//   over the rig
//     warp_aggregate_kernel  observed count, remove_outlier, kept count, mean (:347-358) in camera order
//     (propagation: topo_propagate_kernel of gsr_topo.hip, one call per component)
//     warp_smooth_kernel     one Jacobi sweep of mesh_color_smoothing (ping-pong)
// No float atomics anywhere: every output is a pure function of the inputs (bitwise reproducible, independent of how many
// views are in flight and of how the cameras were sharded over ranks).  Floating point follows the numpy restatement in
// tests/warp_ref.py operation by operation, so contraction into FMAs is off for this file.
//
// Assumptions (cv2 and trimesh are not available to check them against):
//   * cv2.blur(., (7, 7)): BORDER_REFLECT_101, the 49 values summed in double times 1/49 and rounded to f32 -- edge_var of
//     gsr_rig.h, which states the convention once for this filter and the detection's 3x3.
//   * cv2.resize(flow, (W, H), INTER_NEAREST) as OpenCV's resizeNN computes it: source column
//     min(floor(x * (1.0 / ((double)W / w_padded))), w_padded - 1), and the same for rows.
//   * flow *= H / h_padded multiplies in f32 by the f32-rounded ratio (NumPy 1.x value-based casting of the np.float64 scalar,
//     as the reference's environment pins it).
//   * trimesh vertex_normals: a corner-angle-weighted sum of the unit face normals (cross(b - a, c - b), unitised; a face
//     whose cross product has norm <= 1e-12 contributes zero) in ascending face order, then unitised (a zero sum stays zero).
//     Corner angles: arccos of the clipped dot products of the unit edge vectors at corners 0 and 1, pi minus both at corner
//     2, all three zero when one is below 1e-8.  trimesh computes the normals of the camera-space mesh; these are the world
//     normals rotated into the camera, which differ only by rounding.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_rig.h"

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int WP_BLOCK = RIG_BLOCK;   // the rig-wide kernels; the per-camera kernels must run RIG_BLOCK lanes
constexpr int WP_R = 3;          // get_depth_edge(depth, 7): offsets -3 .. 3
constexpr float WP_MAX_DEPTH = 10.f;   // the literal 10 of warp_mesh.py:122 and :319

// blockIdx.y: 0 = depth_cur, 1 = depth_next
__global__ void __launch_bounds__(RIG_BLOCK) warp_depth_max_kernel(int n, const float* __restrict__ cur, const float* __restrict__ nxt,
                                                                   float* __restrict__ parts)
{
    depth_max_pass(n, blockIdx.y ? nxt : cur, WP_MAX_DEPTH, blockIdx.y, parts);
}

__global__ void __launch_bounds__(RIG_BLOCK) warp_var_max_kernel(int H, int W, const float* __restrict__ cur, const float* __restrict__ nxt,
                                                                 float* __restrict__ parts)
{
    var_max_pass<WP_R>(H, W, blockIdx.y ? nxt : cur, blockIdx.y, 2, parts);
}

}  // namespace

// one raw RAFT flow [h, w, 2] f32 in (x, y) order, padded by (top, bottom, left, right) zeros to (hp, wp), scaled by `scale`
// and resized (nearest) to the camera's (H, W); ify / ifx = 1 / (H / hp), 1 / (W / wp) in double as cv2 computes them
struct WarpFlow {
    const float* raw;
    int h, w, top, left, hp, wp;
    float scale;
    double ify, ifx;
};

struct WarpParams {      // warp_config (warp_mesh.py:14-25)
    double normal_cos;   // cmr_view_max_cos
    double edge_scalar, edge_threshold;
    double bi_depth, bi_pix;   // bi_direct_depth_threshold, bi_direct_pix_threshold
    double max_move;     // max_move_dist
};

namespace {

// flow[iy, ix] after pad_and_resize_flow (warp_mesh.py:96-103) and the [..., ::-1] swap (:270-271): (row, col) displacement
__device__ __forceinline__ void wp_flow_at(const WarpFlow& f, int iy, int ix, float& dr, float& dc)
{
    const int sy = min((int)floor((double)iy * f.ify), f.hp - 1);
    const int sx = min((int)floor((double)ix * f.ifx), f.wp - 1);
    const int ry = sy - f.top, rx = sx - f.left;
    if (ry < 0 || ry >= f.h || rx < 0 || rx >= f.w) { dr = 0.f; dc = 0.f; return; }   // np.pad's zeros (times the scale)
    const float* p = f.raw + ((size_t)ry * f.w + rx) * 2;
    dr = p[1] * f.scale;
    dc = p[0] * f.scale;
}

// edge_vis = min(var / max(var) * edge_scalar, 1) in f32 (warp_mesh.py:298, :313)
__device__ __forceinline__ float wp_edge_vis(const float* g, int H, int W, int y, int x, float m, float vmax, float scalar)
{
    return fminf(__fdiv_rn(edge_var<WP_R>(g, H, W, y, x, m), vmax) * scalar, 1.f);
}

__global__ void __launch_bounds__(RIG_BLOCK) warp_view_kernel(int H, int W, int V, const double* __restrict__ verts,
                                                             const double* __restrict__ normals, WarpFlow ff, WarpFlow fb,
                                                             const float* __restrict__ dcur, const float* __restrict__ dnext,
                                                             const float* __restrict__ parts, RigCamera cam, WarpParams prm,
                                                             double* __restrict__ row)
{
    __shared__ float red[RIG_BLOCK];
    const float gmax_c = block_max_of_parts(parts, red);
    const float gmax_n = block_max_of_parts(parts + RIG_PARTS, red);
    const float vmax_c = block_max_of_parts(parts + 2 * RIG_PARTS, red);
    const float vmax_n = block_max_of_parts(parts + 3 * RIG_PARTS, red);
    const int v = blockIdx.x * RIG_BLOCK + threadIdx.x;
    if (v >= V) return;
    double* out = row + 3 * (size_t)v;
    // a camera whose depth has no pixel below 10 (the reference raises on the empty max) or is flat (max(var) = 0: edge_vis
    // is NaN and nothing passes `< edge_threshold`) sees no vertex
    if (gmax_c == -INFINITY || gmax_n == -INFINITY || !(vmax_c > 0.f) || !(vmax_n > 0.f)) {
        out[0] = out[1] = out[2] = NAN;
        return;
    }
    const float m_c = clip_depth(gmax_c), m_n = clip_depth(gmax_n);
    const float escale = (float)prm.edge_scalar, ethr = (float)prm.edge_threshold;
    // 1. project and look up depth_cur (:287-289)
    const double px = verts[3 * v], py = verts[3 * v + 1], pz = verts[3 * v + 2];
    double lx, ly, lz, pr, pc;
    rig_project(cam, H, W, px, py, pz, lx, ly, lz, pr, pc);
    bool ok = true;
    const int iy = rig_query(pr, H, ok), ix = rig_query(pc, W, ok);
    const float d_cur = dcur[(size_t)iy * W + ix];
    // 2. visible: valid lookup, |z - depth| < 0.005, camera-space normal z < cmr_view_max_cos (:291-295), edge (:298-300)
    const double nz = cam.R[6] * normals[3 * v] + cam.R[7] * normals[3 * v + 1] + cam.R[8] * normals[3 * v + 2];
    bool vis = ok && fabs(lz - (double)d_cur) < 0.005 && nz < prm.normal_cos;
    vis = vis && wp_edge_vis(dcur, H, W, iy, ix, m_c, vmax_c, escale) < ethr;
    // 3. pix_next = pix + flow[q(pix)] (:303)
    float fr, fc;
    wp_flow_at(ff, iy, ix, fr, fc);
    const double nr = pr + (double)fr, nc = pc + (double)fc;
    bool ok_n = true;
    const int jy = rig_query(nr, H, ok_n), jx = rig_query(nc, W, ok_n);
    // 4. pix_back = pix_next + flow_back[q(pix_next)] (:306)
    wp_flow_at(fb, jy, jx, fr, fc);
    const double br = nr + (double)fr, bc = nc + (double)fc;
    bool ok_b = true;
    const int ky = rig_query(br, H, ok_b), kx = rig_query(bc, W, ok_b);
    // 5. depth consistency in f32 (:307-308)
    vis = vis && fabsf(dcur[(size_t)ky * W + kx] - d_cur) < (float)prm.bi_depth;
    // 6. pixel round trip in f64 (:309-310)
    const double er = br - pr, ec = bc - pc;
    vis = vis && sqrt(er * er + ec * ec) < prm.bi_pix;
    // 7. edge in the next frame (:313-315)
    vis = vis && wp_edge_vis(dnext, H, W, jy, jx, m_n, vmax_n, escale) < ethr;
    // 8. depth in the next frame (:318-319)
    const float d_next = dnext[(size_t)jy * W + jx];
    vis = vis && ok_n && d_next < WP_MAX_DEPTH;
    // 9. back-project pix_next with that depth (:77-93, :325): R^T (dir d - t)
    const double dd = (double)d_next;
    const double a0 = ((nc - W * 0.5) / cam.fx) * dd - cam.t[0];
    const double a1 = ((nr - H * 0.5) / cam.fy) * dd - cam.t[1];
    const double a2 = dd - cam.t[2];
    const double m0 = (cam.R[0] * a0 + cam.R[3] * a1 + cam.R[6] * a2) - px;
    const double m1 = (cam.R[1] * a0 + cam.R[4] * a1 + cam.R[7] * a2) - py;
    const double m2 = (cam.R[2] * a0 + cam.R[5] * a1 + cam.R[8] * a2) - pz;
    // 10. |move| < max_move_dist (:326-328)
    vis = vis && sqrt(m0 * m0 + m1 * m1 + m2 * m2) < prm.max_move;
    out[0] = vis ? m0 : NAN;
    out[1] = vis ? m1 : NAN;
    out[2] = vis ? m2 : NAN;
}

__device__ __forceinline__ void unitize3(double& x, double& y, double& z)
{
    const double n = sqrt(x * x + y * y + z * z);
    if (n > 1e-12) { x = x / n; y = y / n; z = z / n; }
    else { x = 0.0; y = 0.0; z = 0.0; }
}

// per face: the unit normal and the three corner angles -> fbuf[6 f .. 6 f + 5]
__global__ void __launch_bounds__(WP_BLOCK) warp_face_kernel(int F, const double* __restrict__ verts, const int* __restrict__ faces,
                                                             double* __restrict__ fbuf)
{
    const int f = blockIdx.x * WP_BLOCK + threadIdx.x;
    if (f >= F) return;
    const double* a = verts + 3 * (size_t)faces[3 * f];
    const double* b = verts + 3 * (size_t)faces[3 * f + 1];
    const double* c = verts + 3 * (size_t)faces[3 * f + 2];
    const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
    double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
    unitize3(nx, ny, nz);
    double u[3] = {e1[0], e1[1], e1[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]}, w[3] = {e2[0], e2[1], e2[2]};
    unitize3(u[0], u[1], u[2]);
    unitize3(v[0], v[1], v[2]);
    unitize3(w[0], w[1], w[2]);
    const double uv = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
    const double uw = -u[0] * w[0] + -u[1] * w[1] + -u[2] * w[2];
    double a0 = acos(fmin(fmax(uv, -1.0), 1.0)), a1 = acos(fmin(fmax(uw, -1.0), 1.0));
    double a2 = M_PI - a0 - a1;
    if (a0 < 1e-8 || a1 < 1e-8 || a2 < 1e-8) a0 = a1 = a2 = 0.0;
    double* o = fbuf + 6 * (size_t)f;
    o[0] = nx; o[1] = ny; o[2] = nz;
    o[3] = a0; o[4] = a1; o[5] = a2;
}

// per vertex: sum over its (face, corner) incidences in ascending face order of angle * normal, unitised
__global__ void __launch_bounds__(WP_BLOCK) warp_vertex_normal_kernel(int V, const int* __restrict__ off, const int* __restrict__ ent,
                                                                      const double* __restrict__ fbuf, double* __restrict__ normals)
{
    const int v = blockIdx.x * WP_BLOCK + threadIdx.x;
    if (v >= V) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int e = off[v]; e < off[v + 1]; ++e) {
        const int f = ent[e] / 3, k = ent[e] % 3;
        const double* o = fbuf + 6 * (size_t)f;
        const double a = o[3 + k];
        sx += a * o[0];
        sy += a * o[1];
        sz += a * o[2];
    }
    unitize3(sx, sy, sz);
    normals[3 * v] = sx;
    normals[3 * v + 1] = sy;
    normals[3 * v + 2] = sz;
}

// warp_mesh.py:347-358 per vertex, cameras in order.  remove_outlier(threshold=2) (:174-181): mean and population std of the
// observed moves, z = (x - mean) / std, keep the rows whose three z are all < 2 (one-sided; a NaN z, from std 0, drops the row)
__global__ void __launch_bounds__(WP_BLOCK) warp_aggregate_kernel(int C, int V, const double* __restrict__ table, int min_observe,
                                                                  double* __restrict__ move, int* __restrict__ observed,
                                                                  int* __restrict__ count, unsigned char* __restrict__ valid)
{
    const int v = blockIdx.x * WP_BLOCK + threadIdx.x;
    if (v >= V) return;
    const size_t stride = 3 * (size_t)V;
    const double* col = table + 3 * (size_t)v;
    int n = 0;
    double s[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < C; ++c) {
        const double* x = col + c * stride;
        if (x[0] == x[0]) { s[0] += x[0]; s[1] += x[1]; s[2] += x[2]; ++n; }   // (NaN = not visible)
    }
    int cnt = n;
    double mv[3] = {0.0, 0.0, 0.0};
    if (n >= min_observe) {
        double mean[3], q[3] = {0.0, 0.0, 0.0}, sd[3];
        for (int k = 0; k < 3; ++k) mean[k] = s[k] / n;
        for (int c = 0; c < C; ++c) {
            const double* x = col + c * stride;
            if (x[0] == x[0])
                for (int k = 0; k < 3; ++k) { const double d = x[k] - mean[k]; q[k] += d * d; }
        }
        for (int k = 0; k < 3; ++k) sd[k] = sqrt(q[k] / n);
        int kept = 0;
        double s2[3] = {0.0, 0.0, 0.0};
        for (int c = 0; c < C; ++c) {
            const double* x = col + c * stride;
            if (x[0] == x[0] && (x[0] - mean[0]) / sd[0] < 2.0 && (x[1] - mean[1]) / sd[1] < 2.0 && (x[2] - mean[2]) / sd[2] < 2.0) {
                s2[0] += x[0]; s2[1] += x[1]; s2[2] += x[2];
                ++kept;
            }
        }
        cnt = kept;
        if (kept >= min_observe)
            for (int k = 0; k < 3; ++k) mv[k] = s2[k] / kept;
    }
    for (int k = 0; k < 3; ++k) move[3 * v + k] = mv[k];
    observed[v] = n;
    count[v] = cnt;
    valid[v] = cnt >= min_observe;
}

// one sweep of mesh_color_smoothing (warp_mesh.py:158-171): every vertex takes the mean of all its neighbours (ascending);
// a vertex without neighbours gets 0 / 0 = NaN, as np.average of an empty selection
__global__ void __launch_bounds__(WP_BLOCK) warp_smooth_kernel(int V, const int* __restrict__ off, const int* __restrict__ nbr,
                                                               const double* __restrict__ in, double* __restrict__ out)
{
    const int v = blockIdx.x * WP_BLOCK + threadIdx.x;
    if (v >= V) return;
    double s[3] = {0.0, 0.0, 0.0};
    int k = 0;
    for (int e = off[v]; e < off[v + 1]; ++e) {
        const double* x = in + 3 * (size_t)nbr[e];
        s[0] += x[0]; s[1] += x[1]; s[2] += x[2];
        ++k;
    }
    const double n = (double)k;
    for (int j = 0; j < 3; ++j) out[3 * v + j] = s[j] / n;
}

inline int wblocks(int n) { return (n + WP_BLOCK - 1) / WP_BLOCK; }

WarpFlow make_flow(const float* raw, const int* shape6, int H, int W)
{
    // shape6: h, w, top, bottom, left, right
    WarpFlow f;
    f.raw = raw;
    f.h = shape6[0];
    f.w = shape6[1];
    f.top = shape6[2];
    f.left = shape6[4];
    f.hp = shape6[0] + shape6[2] + shape6[3];
    f.wp = shape6[1] + shape6[4] + shape6[5];
    f.scale = (float)((double)H / (double)f.hp);
    f.ify = 1.0 / ((double)H / (double)f.hp);
    f.ifx = 1.0 / ((double)W / (double)f.wp);
    return f;
}

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

int gsr_vertex_normals(int V, int F, const double* verts, const int* faces, const int* vf_offsets, const int* vf_entries,
                       double* face_scratch, double* normals, gsr_stream_t stream)
{
    clear_error();
    if (V < 0 || F < 0) return fail_msg("gsr_vertex_normals: negative size");
    if (V == 0) return 0;
    if (!verts || !vf_offsets || !normals || (F > 0 && (!faces || !vf_entries || !face_scratch)))
        return fail_msg("gsr_vertex_normals: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    if (F > 0) warp_face_kernel<<<wblocks(F), WP_BLOCK, 0, st>>>(F, verts, faces, face_scratch);
    warp_vertex_normal_kernel<<<wblocks(V), WP_BLOCK, 0, st>>>(V, vf_offsets, vf_entries, face_scratch, normals);
    GSR_CHECK_LAUNCH("warp normal kernels");
    return 0;
}

size_t gsr_warp_view_workspace_bytes(int H, int W)
{
    (void)H; (void)W;   // (the partial maxima of a fixed number of workgroups, whatever the image)
    return 4 * RIG_PARTS * sizeof(float);
}

int gsr_warp_view(int H, int W, int V, const double* verts, const double* normals, const float* flow_f, const float* flow_b,
                  const int* flow_shape, const float* depth_cur, const float* depth_next, const double* cam,
                  const double* params, void* workspace, double* row, gsr_stream_t stream)
{
    clear_error();
    if (H <= 0 || W <= 0 || V < 0) return fail_msg("gsr_warp_view: sizes must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail_msg("gsr_warp_view: image too large");
    if (!flow_f || !flow_b || !flow_shape || !depth_cur || !depth_next || !cam || !params || !workspace ||
        (V > 0 && (!verts || !normals || !row)))
        return fail_msg("gsr_warp_view: required pointer is null");
    if (flow_shape[0] <= 0 || flow_shape[1] <= 0) return fail_msg("gsr_warp_view: flow sizes must be positive");
    for (int i = 2; i < 6; ++i)
        if (flow_shape[i] < 0) return fail_msg("gsr_warp_view: flow padding must be non-negative");
    const long long hp = (long long)flow_shape[0] + flow_shape[2] + flow_shape[3];
    const long long wp = (long long)flow_shape[1] + flow_shape[4] + flow_shape[5];
    if (hp >= (1ll << 30) || wp >= (1ll << 30) || (long long)flow_shape[0] * flow_shape[1] >= (1ll << 30))
        return fail_msg("gsr_warp_view: flow too large");
    hipStream_t st = (hipStream_t)stream;
    float* parts = static_cast<float*>(workspace);
    WarpParams prm;
    prm.normal_cos = params[0];
    prm.edge_scalar = params[1];
    prm.edge_threshold = params[2];
    prm.bi_depth = params[3];
    prm.bi_pix = params[4];
    prm.max_move = params[5];
    const WarpFlow ff = make_flow(flow_f, flow_shape, H, W), fb = make_flow(flow_b, flow_shape, H, W);
    warp_depth_max_kernel<<<dim3(RIG_PARTS, 2), RIG_BLOCK, 0, st>>>(H * W, depth_cur, depth_next, parts);
    warp_var_max_kernel<<<dim3(RIG_PARTS, 2), RIG_BLOCK, 0, st>>>(H, W, depth_cur, depth_next, parts);
    if (V > 0)
        warp_view_kernel<<<wblocks(V), RIG_BLOCK, 0, st>>>(H, W, V, verts, normals, ff, fb, depth_cur, depth_next, parts,
                                                           rig_camera(cam), prm, row);
    GSR_CHECK_LAUNCH("warp view kernels");
    return 0;
}

int gsr_warp_aggregate(int C, int V, const double* table, int min_observe, double* move, int* observed, int* count,
                       unsigned char* valid, gsr_stream_t stream)
{
    clear_error();
    if (C < 0 || V < 0) return fail_msg("gsr_warp_aggregate: negative size");
    if (V == 0) return 0;
    if ((C > 0 && !table) || !move || !observed || !count || !valid) return fail_msg("gsr_warp_aggregate: required pointer is null");
    warp_aggregate_kernel<<<wblocks(V), WP_BLOCK, 0, (hipStream_t)stream>>>(C, V, table, min_observe, move, observed, count, valid);
    GSR_CHECK_LAUNCH("warp_aggregate_kernel");
    return 0;
}

int gsr_warp_smooth(int V, const int* nbr_offsets, const int* nbr, int sweeps, const double* value_in, double* value_out,
                    double* value_tmp, gsr_stream_t stream)
{
    clear_error();
    if (V < 0 || sweeps < 0) return fail_msg("gsr_warp_smooth: negative size");
    if (V == 0) return 0;
    if (!value_in || !value_out) return fail_msg("gsr_warp_smooth: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    if (sweeps == 0) {
        GSR_CHECK(hipMemcpyAsync(value_out, value_in, sizeof(double) * 3 * V, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    if (!nbr_offsets || !nbr || !value_tmp) return fail_msg("gsr_warp_smooth: required pointer is null");
    ping_pong_sweeps(sweeps, value_in, value_out, value_tmp, [&](const double* src, double* dst, int) {
        warp_smooth_kernel<<<wblocks(V), WP_BLOCK, 0, st>>>(V, nbr_offsets, nbr, src, dst);
    });
    GSR_CHECK_LAUNCH("warp_smooth_kernel");
    return 0;
}

}  // extern "C"
