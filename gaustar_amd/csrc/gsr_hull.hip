// gsr_hull.hip -- shape from silhouettes: the visual hull of a calibrated rig's alpha masks as a TSDF volume that
// gsr_fusion.hip's marching cubes reads unchanged (gaustar_amd.hull).  The reference takes its per-frame meshes from HumanRF
// (README.md:38-39), which does not run here; a capture of 160 masked views carves a tight surface without it.
//   per image
//     hull_row_kernel     s [H,W] int8: per pixel the distance along its row to the nearest pixel of the OTHER kind (inside =
//                         mask >= threshold), capped at R, signed + for an inside pixel and - for an outside one; never 0.
//                         One wave per 1024 pixels of a row, 16 pixels a lane: one 16-byte load where the row allows it.  A
//                         lane's 16 inside / outside bits are packed with its three neighbours' into 64-bit words (20 of each
//                         kind in LDS: the segment and 128 pixels on either side, read as broadcasts); the nearest set bit of
//                         the other kind on either side is two count-zero instructions over at most three words.  Pixels
//                         beyond the image set no bit of either kind: they are unknown.
//     hull_col_kernel     d2 [H,W] int16 = +-min(R^2, min over rows y' within R of dy^2 + h^2), h = 0 where the pixel of this
//                         column in row y' is of the other kind, else |s| there.  A workgroup stages (th + 2 R) rows of 64
//                         columns of s in LDS, th = 16 rows for R <= 40, else 64 (16-byte loads and ds writes; a row is 64
//                         bytes, a wave reads 16 consecutive dwords of it: no bank conflict) and walks dy four at a time
//                         until dy^2 reaches the best so far.
//                         Together: the exact squared Euclidean distance to the nearest pixel of the other kind, capped at R^2.
//   per chunk of cameras
//     hull_carve_kernel   one workgroup per 16^3 unit, 256 lanes x 4 trips x 4 voxels (one float4 of `field`, one int4 of
//                         `count`); the camera records are read wave-uniformly from a device table; a voxel keeps its field
//                         and count in registers over the whole chunk.  Per voxel centre p and camera, in f64 without
//                         contraction, in the order include/gsr.h states: q = R p + t; q.z <= znear or a projection off
//                         [0, W-1] x [0, H-1] leaves the voxel alone; else phi = +-(sqrt|d2| - 0.5) at four taps, bilinear,
//                         d = (phi q.z) (2 / (fx + fy)), field = min(field, f32(d)), count += 1.
//   once
//     hull_finish_kernel  weight = count >= min_views, tsdf = f32(clamp(-field / sdf_trunc, -1, 1)) under weight 1 else 0,
//                         touched per unit.
// Everything before the f32 rounding is a pure function of one voxel and one camera, the rounding is monotone and min and +
// commute: the state does not depend on the cameras' order or on how they are split into calls, streams or ranks.  No
// shortcut skips a camera or a voxel.  No atomics of any kind, no scratch.  tests/hull_ref.py restates it all in numpy.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_rig.h"
#include "gsr_volume.h"

#include <cstddef>
#include <cstdint>
#include <string>

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int HD_MAX_R = 127;
constexpr int HD_LANE_PX = 16;                      // pixels of a row per lane: one 16-byte load
constexpr int HD_SEG = 64 * HD_LANE_PX;             // pixels of a row per wave
constexpr int HD_HALO = 128;                        // >= HD_MAX_R + 1 and a multiple of 64: two words on either side
constexpr int HD_WORDS = (HD_SEG + 2 * HD_HALO) / 64;
constexpr int HC_TW = 64, HC_TH = 64;               // the column pass's tile: columns (= lanes) x rows (a quarter per wave)
constexpr int HC_TH_SHORT = 16, HC_SHORT_R = 40;    // rows of a tile while R <= 40
constexpr int HC_BLOCK = 256;
constexpr int HV_BLOCK = 256;
constexpr double HULL_ZNEAR = 0.01;                 // as gaustar_amd.mesh_depth

typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------------- distance, rows
// The distance from bit p to the nearest set bit of w[] on either side, at most R.  p >= 128 and p + 128 < 64 words' bits.
__host__ __device__ __forceinline__ int nearest_set(const u64* w, int p, int R)
{
    const int wi = p >> 6, b = p & 63;
    int best = R;
    u64 m = (w[wi] >> b) >> 1;                       // the bits after p
    if (m) best = min(best, (int)__builtin_ctzll(m) + 1);
    else if ((m = w[wi + 1]) != 0) best = min(best, 64 - b + (int)__builtin_ctzll(m));
    else if ((m = w[wi + 2]) != 0) best = min(best, 128 - b + (int)__builtin_ctzll(m));
    m = w[wi] & (((u64)1 << b) - 1);                 // the bits before p
    if (m) best = min(best, b - 63 + (int)__builtin_clzll(m));
    else if ((m = w[wi - 1]) != 0) best = min(best, b + 1 + (int)__builtin_clzll(m));
    else if ((m = w[wi - 2]) != 0) best = min(best, b + 65 + (int)__builtin_clzll(m));
    return best;
}

// 16 pixels of a row from column x on: bit i of `in` / `out` = pixel x + i is inside / outside; a column off the image is neither
__device__ __forceinline__ void load_kinds(const unsigned char* __restrict__ row, int x, int W, int thr, unsigned& in, unsigned& out)
{
    in = out = 0;
    if (x >= 0 && x + HD_LANE_PX <= W && (reinterpret_cast<uintptr_t>(row + x) & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(row + x);
        const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < HD_LANE_PX; ++i) in |= (unsigned)((int)((q[i >> 2] >> (8 * (i & 3))) & 255u) >= thr) << i;
        out = ~in & 0xFFFFu;
    } else {
#pragma unroll
        for (int i = 0; i < HD_LANE_PX; ++i) {
            const int c = x + i;
            if (c >= 0 && c < W) {
                const unsigned k = (int)row[c] >= thr;
                in |= k << i;
                out |= (k ^ 1u) << i;
            }
        }
    }
}

// four neighbouring lanes' 16 bits as one word, the same value in each of the four
__device__ __forceinline__ u64 pack4(unsigned bits, int lane)
{
    const int base = lane & ~3;
    return (u64)__shfl(bits, base, 64) | ((u64)__shfl(bits, base + 1, 64) << 16) | ((u64)__shfl(bits, base + 2, 64) << 32) |
           ((u64)__shfl(bits, base + 3, 64) << 48);
}

// grid (ceil(W / 1024), H), one wave each
__global__ void __launch_bounds__(64) hull_row_kernel(int H, int W, const unsigned char* __restrict__ mask, int thr, int R,
                                                      signed char* __restrict__ s)
{
    __shared__ u64 words[2][HD_WORDS];               // [0]: inside, [1]: outside; bit p = column x_base - HD_HALO + p
    const int lane = threadIdx.x;
    const int y = blockIdx.y, x_base = blockIdx.x * HD_SEG;
    const unsigned char* row = mask + (size_t)y * W;
    const int x = x_base + HD_LANE_PX * lane;
    unsigned in, out, hin, hout;
    load_kinds(row, x, W, thr, in, out);
    // lanes 0..7: the 128 columns before the segment; lanes 8..15: the 128 after it
    const int hx = lane < 8 ? x_base - HD_HALO + HD_LANE_PX * lane : x_base + HD_SEG + HD_LANE_PX * (lane - 8);
    hin = hout = 0;
    if (lane < 16) load_kinds(row, hx, W, thr, hin, hout);
    const u64 win = pack4(in, lane), wout = pack4(out, lane), whin = pack4(hin, lane), whout = pack4(hout, lane);
    if ((lane & 3) == 0) {
        words[0][2 + (lane >> 2)] = win;
        words[1][2 + (lane >> 2)] = wout;
        if (lane < 16) {
            const int k = lane < 8 ? (lane >> 2) : HD_WORDS - 2 + ((lane - 8) >> 2);
            words[0][k] = whin;
            words[1][k] = whout;
        }
    }
    __syncthreads();
    if (x >= W) return;
    unsigned q[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < HD_LANE_PX; ++i) {
        const int inside = (in >> i) & 1;
        int d = nearest_set(words[inside], HD_HALO + HD_LANE_PX * lane + i, R);   // inside looks for outside bits: words[1]
        d = inside ? d : -d;
        q[i >> 2] |= ((unsigned)d & 255u) << (8 * (i & 3));
    }
    signed char* dst = s + (size_t)y * W + x;
    if (x + HD_LANE_PX <= W && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<uint4*>(dst) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
        for (int i = 0; i < HD_LANE_PX; ++i)
            if (x + i < W) dst[i] = (signed char)((q[i >> 2] >> (8 * (i & 3))) & 255u);
    }
}

// ---------------------------------------------------------------------------------------------------- distance, columns
// grid (ceil(W / 64), ceil(H / th)), th = rows of a tile, a multiple of 4 (a quarter per wave); dynamic LDS (th + 2 R) * 64 bytes.
// Every candidate dy^2 + h^2 is a true squared distance to a pixel of the other kind (or to nothing nearer), so looking at
// four dy at a time -- eight loads in flight instead of two on the dependent chain -- changes nothing but the time.
__global__ void __launch_bounds__(HC_BLOCK) hull_col_kernel(int H, int W, const signed char* __restrict__ s, int R, int th,
                                                            short* __restrict__ d2)
{
    extern __shared__ __align__(16) signed char tile[];   // row r = image row y0 - R + r, 64 columns from x0
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * HC_TW, y0 = blockIdx.y * th;
    const int rows = th + 2 * R;
    for (int r = t >> 2; r < rows; r += HC_BLOCK / 4) {
        const int y = y0 - R + r, x = x0 + 16 * (t & 3);
        if (y < 0 || y >= H || x >= W) continue;          // (never read below: rows off the image and columns of idle lanes)
        const signed char* src = s + (size_t)y * W + x;
        signed char* dst = tile + r * HC_TW + 16 * (t & 3);
        if (x + 16 <= W && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
            *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
        } else {
            for (int k = 0; k < 16 && x + k < W; ++k) dst[k] = src[k];
        }
    }
    __syncthreads();
    const int lane = t & 63, wave = t >> 6;
    const int x = x0 + lane;
    if (x >= W) return;
    const int cap = R * R, per_wave = th / 4;
    for (int i = 0; i < per_wave; ++i) {
        const int ly = wave * per_wave + i, y = y0 + ly;
        if (y >= H) break;
        const signed char* col = tile + (ly + R) * HC_TW + lane;
        const int v = col[0];
        const bool neg = v < 0;
        int best = min(cap, v * v);
        for (int d = 1; d <= R && d * d < best; d += 4) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int dd = d + j;
                if (dd <= R && y - dd >= 0) {
                    const int u = col[-dd * HC_TW];
                    const int h = ((u < 0) == neg) ? u : 0;
                    best = min(best, dd * dd + h * h);
                }
                if (dd <= R && y + dd < H) {
                    const int u = col[dd * HC_TW];
                    const int h = ((u < 0) == neg) ? u : 0;
                    best = min(best, dd * dd + h * h);
                }
            }
        }
        d2[(size_t)y * W + x] = (short)(neg ? -best : best);
    }
}

// ---------------------------------------------------------------------------------------------------- the carve
struct HullCamera {          // 144 bytes; gaustar_amd.hull.CAMERA_DTYPE
    RigPinhole cam;          // world-to-camera (COLMAP axes), focal lengths and principal point
    const short* d2;         // [H,W] int16 on the device: gsr_hull_mask_distance's
    int H, W;
};
static_assert(sizeof(HullCamera) == 144 && offsetof(HullCamera, d2) == 128, "HullCamera is CAMERA_DTYPE's layout");

__host__ __device__ __forceinline__ double hull_phi(int v)
{
    const double r = sqrt((double)(v < 0 ? -v : v)) - 0.5;
    return v < 0 ? -r : r;
}

// one voxel centre and one camera; `scale` = 2.0 / (fx + fy)
__host__ __device__ __forceinline__ void carve_voxel(const HullCamera& c, double scale, double px, double py, double pz, float& field,
                                                     int& count)
{
    double qx, qy, qz;
    rig_local(c.cam.rc, px, py, pz, qx, qy, qz);
    if (!(qz > HULL_ZNEAR)) return;
    double u, v;
    rig_pixel(c.cam.rc.fx, qx, qz, c.cam.cx, u);
    rig_pixel(c.cam.rc.fy, qy, qz, c.cam.cy, v);
    if (!(u >= 0.0 && u <= (double)(c.W - 1) && v >= 0.0 && v <= (double)(c.H - 1))) return;
    const int x0 = min((int)u, c.W - 2), y0 = min((int)v, c.H - 2);   // (u, v >= 0: the conversion is the floor)
    const double a = u - (double)x0, b = v - (double)y0;
    const short* row = c.d2 + (size_t)y0 * c.W + x0;
    const double p00 = hull_phi(row[0]), p01 = hull_phi(row[1]), p10 = hull_phi(row[c.W]), p11 = hull_phi(row[c.W + 1]);
    const double top = p00 + a * (p01 - p00), bot = p10 + a * (p11 - p10);
    const double phi = top + b * (bot - top);
    const float d = (float)((phi * qz) * scale);
    field = d < field ? d : field;
    count += 1;
}

__global__ void __launch_bounds__(HV_BLOCK) hull_carve_kernel(int n, const HullCamera* __restrict__ cams, double voxel, FusionGrid g,
                                                              float* __restrict__ field, int* __restrict__ count)
{
    const int unit = blockIdx.x;
    const int ux = unit % g.nu[0], uy = (unit / g.nu[0]) % g.nu[1], uz = unit / (g.nu[0] * g.nu[1]);
    const size_t nx = (size_t)g.nu[0] * FU, ny = (size_t)g.nu[1] * FU;
    const double L = (double)FU * voxel;
    const double ox = (double)(g.u0[0] + ux) * L, oy = (double)(g.u0[1] + uy) * L, oz = (double)(g.u0[2] + uz) * L;
    for (int q = threadIdx.x; q < FU_QUADS; q += HV_BLOCK) {
        const int x0 = (q & 3) * 4, y = (q >> 2) & (FU - 1), z = q >> 6;
        const size_t at = (((size_t)uz * FU + z) * ny + ((size_t)uy * FU + y)) * nx + (size_t)ux * FU + x0;
        float4 F = *reinterpret_cast<const float4*>(field + at);
        int4 C = *reinterpret_cast<const int4*>(count + at);
        const double cy = oy + ((double)y + 0.5) * voxel, cz = oz + ((double)z + 0.5) * voxel;
        const double c0 = ox + ((double)(x0 + 0) + 0.5) * voxel, c1 = ox + ((double)(x0 + 1) + 0.5) * voxel;
        const double c2 = ox + ((double)(x0 + 2) + 0.5) * voxel, c3 = ox + ((double)(x0 + 3) + 0.5) * voxel;
        for (int k = 0; k < n; ++k) {
            const HullCamera hc = cams[k];
            const double scale = 2.0 / (hc.cam.rc.fx + hc.cam.rc.fy);
            carve_voxel(hc, scale, c0, cy, cz, F.x, C.x);
            carve_voxel(hc, scale, c1, cy, cz, F.y, C.y);
            carve_voxel(hc, scale, c2, cy, cz, F.z, C.z);
            carve_voxel(hc, scale, c3, cy, cz, F.w, C.w);
        }
        *reinterpret_cast<float4*>(field + at) = F;
        *reinterpret_cast<int4*>(count + at) = C;
    }
}

// ---------------------------------------------------------------------------------------------------- finish
__host__ __device__ __forceinline__ float finish_voxel(float field, int count, int min_views, double trunc, float& weight)
{
    if (count < min_views) { weight = 0.f; return 0.f; }
    weight = 1.f;
    const double t = -(double)field / trunc;
    return (float)(t < -1.0 ? -1.0 : (t > 1.0 ? 1.0 : t));
}

__global__ void __launch_bounds__(HV_BLOCK) hull_finish_kernel(FusionGrid g, const float* __restrict__ field, const int* __restrict__ count,
                                                               int min_views, double trunc, float* __restrict__ tsdf,
                                                               float* __restrict__ weight, unsigned char* __restrict__ touched)
{
    const int unit = blockIdx.x;
    const int ux = unit % g.nu[0], uy = (unit / g.nu[0]) % g.nu[1], uz = unit / (g.nu[0] * g.nu[1]);
    const size_t nx = (size_t)g.nu[0] * FU, ny = (size_t)g.nu[1] * FU;
    int any = 0;
    for (int q = threadIdx.x; q < FU_QUADS; q += HV_BLOCK) {
        const int x0 = (q & 3) * 4, y = (q >> 2) & (FU - 1), z = q >> 6;
        const size_t at = (((size_t)uz * FU + z) * ny + ((size_t)uy * FU + y)) * nx + (size_t)ux * FU + x0;
        const float4 F = *reinterpret_cast<const float4*>(field + at);
        const int4 C = *reinterpret_cast<const int4*>(count + at);
        float4 T, Wt;
        T.x = finish_voxel(F.x, C.x, min_views, trunc, Wt.x);
        T.y = finish_voxel(F.y, C.y, min_views, trunc, Wt.y);
        T.z = finish_voxel(F.z, C.z, min_views, trunc, Wt.z);
        T.w = finish_voxel(F.w, C.w, min_views, trunc, Wt.w);
        any |= (Wt.x == 1.f && fabsf(T.x) < 1.f) || (Wt.y == 1.f && fabsf(T.y) < 1.f) || (Wt.z == 1.f && fabsf(T.z) < 1.f) ||
               (Wt.w == 1.f && fabsf(T.w) < 1.f);
        *reinterpret_cast<float4*>(tsdf + at) = T;
        *reinterpret_cast<float4*>(weight + at) = Wt;
    }
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) touched[unit] = any ? 1 : 0;
}

inline bool is_finite(double v) { return v - v == 0.0; }

// the host copy of the camera table, before anything is launched from its device copy
const char* hull_cameras_error(int n, const HullCamera* cams)
{
    for (int k = 0; k < n; ++k) {
        const HullCamera& c = cams[k];
        const RigCamera& rc = c.cam.rc;
        for (int i = 0; i < 9; ++i)
            if (!is_finite(rc.R[i])) return "a camera is not finite";
        if (!is_finite(rc.t[0]) || !is_finite(rc.t[1]) || !is_finite(rc.t[2]) || !is_finite(c.cam.cx) || !is_finite(c.cam.cy)) return "a camera is not finite";
        if (!(rc.fx > 0.0) || !(rc.fy > 0.0) || !is_finite(rc.fx) || !is_finite(rc.fy)) return "focal lengths must be positive and finite";
        if (c.H < 2 || c.W < 2) return "a distance map must be at least 2 x 2";
        if ((long long)c.H * c.W >= (1ll << 31)) return "a distance map is too large";
        if (!c.d2 || (reinterpret_cast<uintptr_t>(c.d2) & 1)) return "a distance map is null or not 2-byte aligned";
    }
    return nullptr;
}

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

size_t gsr_hull_mask_distance_workspace_bytes(int H, int W)
{
    return (H > 0 && W > 0 && (long long)H * W < (1ll << 31)) ? (size_t)H * W : 0;
}

int gsr_hull_mask_distance(int H, int W, const unsigned char* mask, int threshold, int radius, void* workspace, short* d2,
                           gsr_stream_t stream)
{
    clear_error();
    if (H < 2 || W < 2) return fail_msg("gsr_hull_mask_distance: the image must be at least 2 x 2");
    if ((long long)H * W >= (1ll << 31) || H > 65535) return fail_msg("gsr_hull_mask_distance: image too large");
    if (radius < 1 || radius > HD_MAX_R) return fail_msg("gsr_hull_mask_distance: radius must be between 1 and 127");
    if (threshold < 0 || threshold > 256) return fail_msg("gsr_hull_mask_distance: threshold must be between 0 and 256");
    if (!mask || !workspace || !d2) return fail_msg("gsr_hull_mask_distance: required pointer is null");
    if (reinterpret_cast<uintptr_t>(d2) & 1) return fail_msg("gsr_hull_mask_distance: d2 must be 2-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    signed char* s = static_cast<signed char*>(workspace);
    hull_row_kernel<<<dim3((W + HD_SEG - 1) / HD_SEG, H), 64, 0, st>>>(H, W, mask, threshold, radius, s);
    // short tiles while the halo stays a few times the tile (more workgroups than CUs at 1080p), tall ones for a wide halo
    const int th = radius <= HC_SHORT_R ? HC_TH_SHORT : HC_TH;
    const size_t lds = (size_t)(th + 2 * radius) * HC_TW;
    hull_col_kernel<<<dim3((W + HC_TW - 1) / HC_TW, (H + th - 1) / th), HC_BLOCK, lds, st>>>(H, W, s, radius, th, d2);
    GSR_CHECK_LAUNCH("hull distance kernels");
    return 0;
}

int gsr_hull_camera_bytes(void) { return (int)sizeof(HullCamera); }

int gsr_hull_carve(int n_cameras, const void* cameras_host, const void* cameras, double voxel_size, const int* grid, float* field,
                   int* count, gsr_stream_t stream)
{
    clear_error();
    if (n_cameras < 0) return fail_msg("gsr_hull_carve: negative size");
    if (!(voxel_size > 0.0) || !is_finite(voxel_size)) return fail_msg("gsr_hull_carve: voxel_size must be positive");
    if (const char* e = fusion_grid_error(grid)) return fail_msg((std::string("gsr_hull_carve: ") + e).c_str());
    if (!field || !count) return fail_msg("gsr_hull_carve: required pointer is null");
    if ((reinterpret_cast<uintptr_t>(field) | reinterpret_cast<uintptr_t>(count)) & 15)
        return fail_msg("gsr_hull_carve: the volume's arrays must be 16-byte aligned");
    if (n_cameras == 0) return 0;
    if (!cameras_host || !cameras) return fail_msg("gsr_hull_carve: required pointer is null");
    if (reinterpret_cast<uintptr_t>(cameras) & 7) return fail_msg("gsr_hull_carve: the camera table must be 8-byte aligned");
    if (const char* e = hull_cameras_error(n_cameras, static_cast<const HullCamera*>(cameras_host)))
        return fail_msg((std::string("gsr_hull_carve: ") + e).c_str());
    const FusionGrid g = fusion_grid(grid);
    hull_carve_kernel<<<g.nu[0] * g.nu[1] * g.nu[2], HV_BLOCK, 0, (hipStream_t)stream>>>(
        n_cameras, static_cast<const HullCamera*>(cameras), voxel_size, g, field, count);
    GSR_CHECK_LAUNCH("hull_carve_kernel");
    return 0;
}

int gsr_hull_finish(const int* grid, const float* field, const int* count, int min_views, double sdf_trunc, float* tsdf, float* weight,
                    unsigned char* touched, gsr_stream_t stream)
{
    clear_error();
    if (const char* e = fusion_grid_error(grid)) return fail_msg((std::string("gsr_hull_finish: ") + e).c_str());
    if (min_views < 1) return fail_msg("gsr_hull_finish: min_views must be at least 1");
    if (!(sdf_trunc > 0.0) || !is_finite(sdf_trunc)) return fail_msg("gsr_hull_finish: sdf_trunc must be positive");
    if (!field || !count || !tsdf || !weight || !touched) return fail_msg("gsr_hull_finish: required pointer is null");
    if ((reinterpret_cast<uintptr_t>(field) | reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(tsdf) |
         reinterpret_cast<uintptr_t>(weight)) & 15)
        return fail_msg("gsr_hull_finish: the volume's arrays must be 16-byte aligned");
    const FusionGrid g = fusion_grid(grid);
    hull_finish_kernel<<<g.nu[0] * g.nu[1] * g.nu[2], HV_BLOCK, 0, (hipStream_t)stream>>>(g, field, count, min_views, sdf_trunc, tsdf,
                                                                                        weight, touched);
    GSR_CHECK_LAUNCH("hull_finish_kernel");
    return 0;
}

}  // extern "C"
