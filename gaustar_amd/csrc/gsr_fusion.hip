// gsr_fusion.hip -- TSDF fusion of the rig's renders and mesh extraction (gaustar_trainers/refined_mesh.py:311-459,
// `extract_mesh_fusion`): the surface that update_mesh_topo cuts its patches from once detect_topo_err has switched loose
// binding on.
//
// The reference pulls every render to the host, prepares it with numpy / cv2 (:412-445) and integrates it into Open3D's legacy
// ScalableTSDFVolume(voxel_length, sdf_trunc, RGB8) on the CPU, then extracts the mesh with Open3D's marching cubes.  Here:
//   per camera
//     fusion_depth_kernel     depth = ch0 / (alpha + 1e-8), alpha < 0.5 -> 0                         (:412-423)
//     fusion_gt_max_kernel / fusion_var_max_kernel   the two image passes of gsr_rig.h over that depth (get_depth_edge(depth, 3))
//     fusion_prep_kernel      edge_vis > 0.5 -> 0, depth >= depth_trunc -> 0, rgb -> uint8 by truncation (:425-445)
//     fusion_touch_kernel     every 4th pixel of every 4th row: the 16^3-voxel units within sdf_trunc of its world point
//     fusion_integrate_kernel one workgroup per unit of the dense directory, touched units only: the running means
//   once
//     fusion_count_kernel     per voxel: which of its three edges carry a vertex, how many triangles its cube has
//     fusion_emit_kernel      vertices, colours and triangles at the ids an exclusive scan of those counts gives
// The volume is a dense grid over the model's bounding box, x fastest, structure of arrays (tsdf, weight, three colour planes:
// 20 bytes per voxel); a unit's row of 16 voxels is 64 contiguous bytes, read and written as float4.  Open3D's volume is an
// unbounded hash of units: what falls outside the box is dropped here.  Open3D keeps the colour mean in double; it is f32
// here, as tsdf and weight are.  Open3D is not installed where this was written: the rules are those stated in
// tests/fusion_ref.py, and parity with Open3D itself is not pinned.
// No float atomics: touched flags are plain stores of 1, every voxel is written by one lane, vertex and triangle ids come
// from a scan in voxel order -- every output is a pure function of the inputs and of the order of the views.
//
// Floating point follows the numpy restatement in tests/fusion_ref.py operation by operation, so contraction into FMAs is off.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_rig.h"
#include "gsr_volume.h"
#include <string>

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int FU_STRIDE = 4;       // depth_sampling_stride

struct FusionCamera {
    double E[12];    // world-to-camera (COLMAP axes), rows of [R | t]
    double Ei[12];   // its inverse (inverted on the host in double), rows of [R' | t']
    double fx, fy, cx, cy;
};

inline FusionCamera fusion_camera(const double* cam28)
{
    FusionCamera c;
    for (int i = 0; i < 12; ++i) { c.E[i] = cam28[i]; c.Ei[i] = cam28[12 + i]; }
    c.fx = cam28[24]; c.fy = cam28[25]; c.cx = cam28[26]; c.cy = cam28[27];
    return c;
}

// ---------------------------------------------------------------------------------------------------- image preparation
__global__ void __launch_bounds__(RIG_BLOCK) fusion_depth_kernel(int n, const float* __restrict__ ch0, const float* __restrict__ alpha,
                                                                 int mask_background, float* __restrict__ depth)
{
    const int i = blockIdx.x * RIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float a = alpha[i];
    float d = __fdiv_rn(ch0[i], a + 1e-8f);
    if (mask_background && a < 0.5f) d = 0.f;
    depth[i] = d;
}

__global__ void __launch_bounds__(RIG_BLOCK) fusion_gt_max_kernel(int n, const float* __restrict__ depth, float* __restrict__ parts)
{
    depth_max_pass(n, depth, 10.f, 0, parts);   // get_depth_edge(max_depth=None): depth[depth < 10]
}

__global__ void __launch_bounds__(RIG_BLOCK) fusion_var_max_kernel(int H, int W, const float* __restrict__ depth, float* __restrict__ parts)
{
    var_max_pass<1>(H, W, depth, 0, 1, parts);
}

// parts: null without edge removal.  A map without a pixel below 10 (the reference raises on the empty max) or a flat one
// (max(var) = 0: edge_vis is NaN and nothing passes `> 0.5`) loses no pixel to the edge test.
__global__ void __launch_bounds__(RIG_BLOCK) fusion_prep_kernel(int H, int W, const float* __restrict__ depth0, const float* __restrict__ rgb,
                                                                const float* __restrict__ parts, float depth_trunc,
                                                                float* __restrict__ depth, unsigned char* __restrict__ rgb8)
{
    __shared__ float red[RIG_BLOCK];
    float gmax = -INFINITY, vmax = 0.f;
    if (parts) {
        gmax = block_max_of_parts(parts, red);
        vmax = block_max_of_parts(parts + RIG_PARTS, red);
    }
    const int n = H * W;
    const int i = blockIdx.x * RIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    float d = depth0[i];
    if (gmax != -INFINITY && vmax > 0.f) {
        const float var = edge_var<1>(depth0, H, W, i / W, i % W, clip_depth(gmax));
        const float ev = fminf(__fdiv_rn(var, vmax) * 1000.f, 1.f);   // refined_mesh.py:427
        if (ev > 0.5f) d = 0.f;                                       // :430-431
    }
    if (d >= depth_trunc) d = 0.f;   // open3d RGBDImage::CreateFromColorAndDepth
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = fminf(fmaxf(rgb[(size_t)c * n + i], 0.f), 1.f);   // :360 clamp
        rgb8[3 * (size_t)i + c] = (unsigned char)(int)(v * 255.f);        // :441 np.uint8 truncates
    }
    depth[i] = d;
}

// ---------------------------------------------------------------------------------------------------- integration
__global__ void __launch_bounds__(RIG_BLOCK) fusion_touch_kernel(int H, int W, const float* __restrict__ depth, FusionCamera cam,
                                                                 double voxel, double trunc, FusionGrid g,
                                                                 unsigned char* __restrict__ touched)
{
    const int ws = (W + FU_STRIDE - 1) / FU_STRIDE, hs = (H + FU_STRIDE - 1) / FU_STRIDE;
    const int s = blockIdx.x * RIG_BLOCK + threadIdx.x;
    if (s >= ws * hs) return;
    const int i = (s / ws) * FU_STRIDE, j = (s % ws) * FU_STRIDE;
    const float df = depth[(size_t)i * W + j];
    if (!(df > 0.f)) return;
    const double d = (double)df;
    const double x = ((double)j - cam.cx) * d / cam.fx, y = ((double)i - cam.cy) * d / cam.fy;
    const double L = (double)FU * voxel;
    int lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double p = cam.Ei[4 * a] * x + cam.Ei[4 * a + 1] * y + cam.Ei[4 * a + 2] * d + cam.Ei[4 * a + 3];
        const double l = floor((p - trunc) / L), h = floor((p + trunc) / L);
        if (!(l >= (double)g.u0[a] - 1e9 && h <= (double)g.u0[a] + 1e9)) return;   // (not finite, or far outside: nothing)
        lo[a] = max((int)(l - (double)g.u0[a]), 0);
        hi[a] = min((int)(h - (double)g.u0[a]), g.nu[a] - 1);
    }
    for (int uz = lo[2]; uz <= hi[2]; ++uz)
        for (int uy = lo[1]; uy <= hi[1]; ++uy)
            for (int ux = lo[0]; ux <= hi[0]; ++ux) touched[((size_t)uz * g.nu[1] + uy) * g.nu[0] + ux] = 1;
}

// one voxel of one view: the rules of tests/fusion_ref.py (open3d UniformTSDFVolume::IntegrateWithDepthToCameraDistanceMultiplier
// with the multiplier computed in place)
__device__ __forceinline__ void integrate_voxel(const FusionCamera& cam, int H, int W, const float* __restrict__ depth,
                                                const unsigned char* __restrict__ rgb8, float truncf, double cx, double cy,
                                                double cz, float& tsdf, float& w, float& r, float& gch, float& b)
{
    const double X = cam.E[0] * cx + cam.E[1] * cy + cam.E[2] * cz + cam.E[3];
    const double Y = cam.E[4] * cx + cam.E[5] * cy + cam.E[6] * cz + cam.E[7];
    const double Z = cam.E[8] * cx + cam.E[9] * cy + cam.E[10] * cz + cam.E[11];
    if (!(Z > 0.0)) return;
    const double uf = cam.fx * X / Z + cam.cx + 0.5, vf = cam.fy * Y / Z + cam.cy + 0.5;
    if (!(uf >= 1e-4 && uf < (double)W - 1e-4 && vf >= 1e-4 && vf < (double)H - 1e-4)) return;
    const int u = (int)uf, v = (int)vf;   // in [0, W - 1] x [0, H - 1] by the test above
    const size_t p = (size_t)v * W + u;
    const float d = depth[p];
    if (!(d > 0.f)) return;
    const float a = __fdiv_rn((float)u - (float)cam.cx, (float)cam.fx), c = __fdiv_rn((float)v - (float)cam.cy, (float)cam.fy);
    // sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the intrinsic is the native v_sqrt_f32 (1 ulp), while
    // sqrtf is the correctly rounded one numpy computes (clang's default -fhip-fp32-correctly-rounded-divide-sqrt)
    const float sdf = (d - (float)Z) * sqrtf(a * a + c * c + 1.f);
    if (!(sdf > -truncf)) return;
    const float t = fminf(1.f, __fdiv_rn(sdf, truncf));
    const float w1 = w + 1.f;
    tsdf = __fdiv_rn(tsdf * w + t, w1);
    r = __fdiv_rn(r * w + (float)rgb8[3 * p], w1);
    gch = __fdiv_rn(gch * w + (float)rgb8[3 * p + 1], w1);
    b = __fdiv_rn(b * w + (float)rgb8[3 * p + 2], w1);
    w = w1;
}

// grid: one workgroup per unit of the directory; 256 lanes x 4 trips x 4 voxels (one float4 per plane) = 16^3
__global__ void __launch_bounds__(RIG_BLOCK) fusion_integrate_kernel(int H, int W, const float* __restrict__ depth,
                                                                     const unsigned char* __restrict__ rgb8, FusionCamera cam,
                                                                     double voxel, float truncf, FusionGrid g,
                                                                     const unsigned char* __restrict__ touched,
                                                                     float* __restrict__ tsdf, float* __restrict__ weight,
                                                                     float* __restrict__ color)
{
    const int unit = blockIdx.x;
    if (!touched[unit]) return;
    const int ux = unit % g.nu[0], uy = (unit / g.nu[0]) % g.nu[1], uz = unit / (g.nu[0] * g.nu[1]);
    const size_t nx = (size_t)g.nu[0] * FU, ny = (size_t)g.nu[1] * FU;
    const size_t plane = nx * ny * ((size_t)g.nu[2] * FU);
    const double L = (double)FU * voxel;
    const double ox = (double)(g.u0[0] + ux) * L, oy = (double)(g.u0[1] + uy) * L, oz = (double)(g.u0[2] + uz) * L;
    for (int q = threadIdx.x; q < FU_QUADS; q += RIG_BLOCK) {
        const int x0 = (q & 3) * 4, y = (q >> 2) & (FU - 1), z = q >> 6;
        const size_t at = (((size_t)uz * FU + z) * ny + ((size_t)uy * FU + y)) * nx + (size_t)ux * FU + x0;
        float4 T = *reinterpret_cast<const float4*>(tsdf + at);
        float4 Wt = *reinterpret_cast<const float4*>(weight + at);
        float4 R = *reinterpret_cast<const float4*>(color + at);
        float4 G = *reinterpret_cast<const float4*>(color + plane + at);
        float4 B = *reinterpret_cast<const float4*>(color + 2 * plane + at);
        const double cy = oy + ((double)y + 0.5) * voxel, cz = oz + ((double)z + 0.5) * voxel;
        integrate_voxel(cam, H, W, depth, rgb8, truncf, ox + ((double)(x0 + 0) + 0.5) * voxel, cy, cz, T.x, Wt.x, R.x, G.x, B.x);
        integrate_voxel(cam, H, W, depth, rgb8, truncf, ox + ((double)(x0 + 1) + 0.5) * voxel, cy, cz, T.y, Wt.y, R.y, G.y, B.y);
        integrate_voxel(cam, H, W, depth, rgb8, truncf, ox + ((double)(x0 + 2) + 0.5) * voxel, cy, cz, T.z, Wt.z, R.z, G.z, B.z);
        integrate_voxel(cam, H, W, depth, rgb8, truncf, ox + ((double)(x0 + 3) + 0.5) * voxel, cy, cz, T.w, Wt.w, R.w, G.w, B.w);
        *reinterpret_cast<float4*>(tsdf + at) = T;
        *reinterpret_cast<float4*>(weight + at) = Wt;
        *reinterpret_cast<float4*>(color + at) = R;
        *reinterpret_cast<float4*>(color + plane + at) = G;
        *reinterpret_cast<float4*>(color + 2 * plane + at) = B;
    }
}

// ---------------------------------------------------------------------------------------------------- extraction
// Cube corner i sits at (i & 1, i >> 1 & 1, i >> 2) from the cube's voxel; edge e = 4 axis + j runs along `axis` from the corner
// whose two other coordinates (ascending axis order) are (j & 1, j >> 1) -- fusion.mc_table()'s numbering.
struct Dims { int nx, ny, nz; };

__device__ __forceinline__ size_t vox(const Dims& d, int x, int y, int z) { return ((size_t)z * d.ny + y) * d.nx + x; }

__device__ __forceinline__ bool cube_valid(const Dims& d, const float* __restrict__ weight, int x, int y, int z)
{
    if (x < 0 || y < 0 || z < 0 || x + 1 >= d.nx || y + 1 >= d.ny || z + 1 >= d.nz) return false;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) ok = ok && weight[vox(d, x + (i & 1), y + ((i >> 1) & 1), z + (i >> 2))] != 0.f;
    return ok;
}

__device__ __forceinline__ int cube_case(const Dims& d, const float* __restrict__ tsdf, int x, int y, int z)
{
    int c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) c |= (tsdf[vox(d, x + (i & 1), y + ((i >> 1) & 1), z + (i >> 2))] < 0.f) << i;
    return c;
}

__device__ __forceinline__ void edge_others(int axis, int& b, int& c)
{
    b = axis == 0 ? 1 : 0;
    c = axis == 2 ? 1 : 2;
}

__global__ void __launch_bounds__(RIG_BLOCK) fusion_count_kernel(Dims d, const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                                 const int* __restrict__ table, unsigned char* __restrict__ edge_mask,
                                                                 int* __restrict__ vert_count, int* __restrict__ tri_count)
{
    const size_t n = (size_t)d.nx * d.ny * d.nz;
    const size_t i = (size_t)blockIdx.x * RIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    int mask = 0, tris = 0;
    if (weight[i] != 0.f) {   // (every cube around one of this voxel's edges, and its own cube, has this voxel as a corner)
        const int x = (int)(i % d.nx), y = (int)((i / d.nx) % d.ny), z = (int)(i / ((size_t)d.nx * d.ny));
        const bool in = tsdf[i] < 0.f;
        const int p[3] = {x, y, z}, dim[3] = {d.nx, d.ny, d.nz};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (p[a] + 1 >= dim[a]) continue;
            int q[3] = {x, y, z};
            q[a] += 1;
            const size_t j = vox(d, q[0], q[1], q[2]);
            if (weight[j] == 0.f || (tsdf[j] < 0.f) == in) continue;
            int b, c;
            edge_others(a, b, c);
            bool any = false;
            for (int k = 0; k < 4 && !any; ++k) {
                int o[3] = {x, y, z};
                o[b] -= k & 1;
                o[c] -= k >> 1;
                any = cube_valid(d, weight, o[0], o[1], o[2]);
            }
            if (any) mask |= 1 << a;
        }
        if (cube_valid(d, weight, x, y, z)) {
            const int* row = table + 16 * cube_case(d, tsdf, x, y, z);
            while (tris < 5 && row[3 * tris] >= 0) ++tris;
        }
    }
    edge_mask[i] = (unsigned char)mask;
    vert_count[i] = __popc(mask);
    tri_count[i] = tris;
}

__device__ __forceinline__ float voxel_centre(const FusionGrid& g, double voxel, int a, int k)
{
    // unit origin + (index in the unit + 0.5) voxel, in double, rounded to f32 once
    return (float)((double)(g.u0[a] + k / FU) * ((double)FU * voxel) + ((double)(k % FU) + 0.5) * voxel);
}

// vert_scan / tri_scan: the inclusive scans of vert_count / tri_count in voxel order
__global__ void __launch_bounds__(RIG_BLOCK) fusion_emit_kernel(Dims d, FusionGrid g, double voxel, const float* __restrict__ tsdf,
                                                                const float* __restrict__ color,
                                                                const unsigned char* __restrict__ edge_mask,
                                                                const int* __restrict__ vert_scan, const int* __restrict__ tri_scan,
                                                                const int* __restrict__ table, float* __restrict__ verts,
                                                                int* __restrict__ faces, float* __restrict__ colors)
{
    const size_t n = (size_t)d.nx * d.ny * d.nz;
    const size_t i = (size_t)blockIdx.x * RIG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int mask = edge_mask[i];
    const int t0 = i ? tri_scan[i - 1] : 0, nt = tri_scan[i] - t0;
    if (!mask && !nt) return;
    const int x = (int)(i % d.nx), y = (int)((i / d.nx) % d.ny), z = (int)(i / ((size_t)d.nx * d.ny));
    if (mask) {
        int id = i ? vert_scan[i - 1] : 0;
        const float pa[3] = {voxel_centre(g, voxel, 0, x), voxel_centre(g, voxel, 1, y), voxel_centre(g, voxel, 2, z)};
        const float fa = tsdf[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!(mask >> a & 1)) continue;
            int q[3] = {x, y, z};
            q[a] += 1;
            const size_t j = vox(d, q[0], q[1], q[2]);
            const float t = __fdiv_rn(fa, fa - tsdf[j]);
            const float pb = voxel_centre(g, voxel, a, q[a]);
#pragma unroll
            for (int k = 0; k < 3; ++k) verts[3 * (size_t)id + k] = k == a ? pa[a] + t * (pb - pa[a]) : pa[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float ca = color[(size_t)k * n + i], cb = color[(size_t)k * n + j];
                colors[3 * (size_t)id + k] = __fdiv_rn(ca + t * (cb - ca), 255.f);
            }
            ++id;
        }
    }
    if (nt) {
        const int* row = table + 16 * cube_case(d, tsdf, x, y, z);
        for (int k = 0; k < 3 * nt; ++k) {
            const int e = row[k], a = e >> 2, jj = e & 3;
            // (edge_others spelled out: `a` is not a compile-time constant here, and an indexed array would live in scratch)
            const int lo = jj & 1, hi = jj >> 1;
            const size_t owner = vox(d, x + (a == 0 ? 0 : lo), y + (a == 0 ? lo : a == 1 ? 0 : hi), z + (a == 2 ? 0 : hi));
            const int base = owner ? vert_scan[owner - 1] : 0;
            faces[3 * (size_t)t0 + k] = base + __popc(edge_mask[owner] & ((1 << a) - 1));
        }
    }
}

inline int blocks(size_t n) { return (int)((n + RIG_BLOCK - 1) / RIG_BLOCK); }

inline Dims dims_of(const FusionGrid& g) { return Dims{g.nu[0] * FU, g.nu[1] * FU, g.nu[2] * FU}; }

// gsr_fusion_touch: clears the flags, then marks
hipError_t launch_fusion_touch(int H, int W, const float* depth, const double* cam28, double voxel, double trunc, const int* grid6,
                               unsigned char* touched, hipStream_t st)
{
    const FusionGrid g = fusion_grid(grid6);
    const hipError_t e = hipMemsetAsync(touched, 0, (size_t)g.nu[0] * g.nu[1] * g.nu[2], st);
    if (e != hipSuccess) return e;
    const int ns = ((W + FU_STRIDE - 1) / FU_STRIDE) * ((H + FU_STRIDE - 1) / FU_STRIDE);
    fusion_touch_kernel<<<blocks(ns), RIG_BLOCK, 0, st>>>(H, W, depth, fusion_camera(cam28), voxel, trunc, g, touched);
    return hipSuccess;
}

bool fusion_camera_ok(const double* cam)
{
    if (!cam) return false;
    for (int i = 0; i < 28; ++i)
        if (!(cam[i] - cam[i] == 0.0)) return false;
    return cam[24] != 0.0 && cam[25] != 0.0;
}

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

size_t gsr_fusion_prep_workspace_bytes(int H, int W)
{
    return (H > 0 && W > 0 && (long long)H * W < (1ll << 31)) ? 2 * RIG_PARTS * sizeof(float) + (size_t)H * W * sizeof(float) : 0;
}

size_t gsr_fusion_volume_bytes(const int* grid)
{
    if (fusion_grid_error(grid)) return 0;
    return (size_t)grid[3] * grid[4] * grid[5] * 4096 * 20;
}

int gsr_fusion_prep(int H, int W, const float* depth_alpha, const float* rgb, int mask_background, int remove_depth_edge,
                    float depth_trunc, void* workspace, float* depth, unsigned char* rgb8, gsr_stream_t stream)
{
    clear_error();
    if (H <= 0 || W <= 0) return fail_msg("gsr_fusion_prep: sizes must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail_msg("gsr_fusion_prep: image too large");
    if (!depth_alpha || !rgb || !workspace || !depth || !rgb8) return fail_msg("gsr_fusion_prep: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    float* parts = static_cast<float*>(workspace);
    float* depth0 = parts + 2 * RIG_PARTS;
    const int n = H * W;
    fusion_depth_kernel<<<blocks(n), RIG_BLOCK, 0, st>>>(n, depth_alpha, depth_alpha + 2 * (size_t)n, mask_background != 0, depth0);
    if (remove_depth_edge) {
        fusion_gt_max_kernel<<<RIG_PARTS, RIG_BLOCK, 0, st>>>(n, depth0, parts);
        fusion_var_max_kernel<<<RIG_PARTS, RIG_BLOCK, 0, st>>>(H, W, depth0, parts);
    }
    fusion_prep_kernel<<<blocks(n), RIG_BLOCK, 0, st>>>(H, W, depth0, rgb, remove_depth_edge ? parts : nullptr, depth_trunc, depth, rgb8);
    GSR_CHECK_LAUNCH("fusion prep kernels");
    return 0;
}

int gsr_fusion_touch(int H, int W, const float* depth, const double* cam, double voxel_size, double sdf_trunc, const int* grid,
                     unsigned char* touched, gsr_stream_t stream)
{
    clear_error();
    if (H <= 0 || W <= 0) return fail_msg("gsr_fusion_touch: sizes must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail_msg("gsr_fusion_touch: image too large");
    if (!(voxel_size > 0.0) || !(sdf_trunc > 0.0)) return fail_msg("gsr_fusion_touch: voxel_size and sdf_trunc must be positive");
    if (const char* e = fusion_grid_error(grid)) return fail_msg((std::string("gsr_fusion_touch: ") + e).c_str());
    if (!fusion_camera_ok(cam)) return fail_msg("gsr_fusion_touch: camera is null or not finite");
    if (!depth || !touched) return fail_msg("gsr_fusion_touch: required pointer is null");
    GSR_CHECK(launch_fusion_touch(H, W, depth, cam, voxel_size, sdf_trunc, grid, touched, (hipStream_t)stream));
    GSR_CHECK_LAUNCH("fusion_touch_kernel");
    return 0;
}

int gsr_fusion_integrate(int H, int W, const float* depth, const unsigned char* rgb8, const double* cam, double voxel_size,
                         double sdf_trunc, const int* grid, const unsigned char* touched, float* tsdf, float* weight, float* color,
                         gsr_stream_t stream)
{
    clear_error();
    if (H <= 0 || W <= 0) return fail_msg("gsr_fusion_integrate: sizes must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail_msg("gsr_fusion_integrate: image too large");
    if (!(voxel_size > 0.0) || !(sdf_trunc > 0.0)) return fail_msg("gsr_fusion_integrate: voxel_size and sdf_trunc must be positive");
    if (const char* e = fusion_grid_error(grid)) return fail_msg((std::string("gsr_fusion_integrate: ") + e).c_str());
    if (!fusion_camera_ok(cam)) return fail_msg("gsr_fusion_integrate: camera is null or not finite");
    if (!depth || !rgb8 || !touched || !tsdf || !weight || !color) return fail_msg("gsr_fusion_integrate: required pointer is null");
    if ((reinterpret_cast<uintptr_t>(tsdf) | reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(color)) & 15)
        return fail_msg("gsr_fusion_integrate: the volume's arrays must be 16-byte aligned");
    const FusionGrid g = fusion_grid(grid);
    fusion_integrate_kernel<<<g.nu[0] * g.nu[1] * g.nu[2], RIG_BLOCK, 0, (hipStream_t)stream>>>(
        H, W, depth, rgb8, fusion_camera(cam), voxel_size, (float)sdf_trunc, g, touched, tsdf, weight, color);
    GSR_CHECK_LAUNCH("fusion_integrate_kernel");
    return 0;
}

int gsr_fusion_count(const int* grid, const float* tsdf, const float* weight, const int* table, unsigned char* edge_mask,
                     int* vert_count, int* tri_count, gsr_stream_t stream)
{
    clear_error();
    if (const char* e = fusion_grid_error(grid)) return fail_msg((std::string("gsr_fusion_count: ") + e).c_str());
    if (!tsdf || !weight || !table || !edge_mask || !vert_count || !tri_count) return fail_msg("gsr_fusion_count: required pointer is null");
    const Dims d = dims_of(fusion_grid(grid));
    fusion_count_kernel<<<blocks((size_t)d.nx * d.ny * d.nz), RIG_BLOCK, 0, (hipStream_t)stream>>>(d, tsdf, weight, table, edge_mask,
                                                                                                   vert_count, tri_count);
    GSR_CHECK_LAUNCH("fusion_count_kernel");
    return 0;
}

int gsr_fusion_emit(const int* grid, double voxel_size, const float* tsdf, const float* color, const unsigned char* edge_mask,
                    const int* vert_scan, const int* tri_scan, const int* table, float* verts, int* faces, float* colors,
                    gsr_stream_t stream)
{
    clear_error();
    if (const char* e = fusion_grid_error(grid)) return fail_msg((std::string("gsr_fusion_emit: ") + e).c_str());
    if (!(voxel_size > 0.0)) return fail_msg("gsr_fusion_emit: voxel_size must be positive");
    // (verts / faces / colors may be null when the scans' totals are zero: nothing is written then)
    if (!tsdf || !color || !edge_mask || !vert_scan || !tri_scan || !table) return fail_msg("gsr_fusion_emit: required pointer is null");
    const FusionGrid g = fusion_grid(grid);
    const Dims d = dims_of(g);
    fusion_emit_kernel<<<blocks((size_t)d.nx * d.ny * d.nz), RIG_BLOCK, 0, (hipStream_t)stream>>>(
        d, g, voxel_size, tsdf, color, edge_mask, vert_scan, tri_scan, table, verts, faces, colors);
    GSR_CHECK_LAUNCH("fusion_emit_kernel");
    return 0;
}

}  // extern "C"
