// gsr_stereo.hip -- plane-sweep stereo behind a depth prior: the photo-consistency refinement of the visual hull
// (gaustar_amd.stereo).  A hull closes over every concavity (gsr_hull.hip); the rig's colour images see into them.  The prior
// bounds the surface from outside, so per reference camera a short band of fronto-parallel planes behind the prior's depth is
// swept, each plane scored by the normalised cross-correlation of the reference window with the sources' warped windows.
//   per image
//     stereo_luma_kernel         Y = (77 R + 150 G + 29 B + 128) >> 8.  Four pixels a lane: three dwords in, one dword out where
//                                both images are 4-byte aligned, bytes elsewhere and in the tail.
//   per reference camera
//     stereo_sweep_kernel<R>     one workgroup of 256 lanes per 16 x 16 tile.  Planes are global per camera, z_k = k step, so a
//                                tile's lanes share them: the tile's plane range is the union of its pixels' bands (a wave
//                                shuffle, then four words of LDS: no atomics), and per plane the S warped (16 + 2 R)^2 patches
//                                are made ONCE by the whole workgroup into LDS as f64 (an invalid warp is -1; a valid one is
//                                >= 0, so the sign is the valid bit), source by source so that a source's record is read
//                                wave-uniformly.  After one barrier every lane whose own band holds the plane runs its N-tap
//                                sums from LDS.  The projection and the bilinear taps are done 1 / N as often as per tap.
//                                A lane keeps the best cost, its plane, the previous cost and the costs beside the best in
//                                registers; the S scores of a plane pass through an eight-entry insertion network (static
//                                indices: registers, no scratch).
//   after all sweeps
//     stereo_consistency_kernel  one lane per pixel: an accepted depth must be met by the accepted depths of its sources.
//   per volume
//     stereo_merge_kernel        one workgroup per 16^3 unit, float4 accesses: the hull's TSDF carved by the stereo volume's.
// Everything is f64 without contraction in the order include/gsr.h states; no atomics of any kind, no scratch; every output is
// a pure function of the inputs.  tests/stereo_ref.py restates it all in numpy.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_rig.h"
#include "gsr_volume.h"

#include <climits>
#include <cstddef>
#include <cstdint>
#include <string>

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int SV_TILE = 16;
constexpr int SV_BLOCK = SV_TILE * SV_TILE;
constexpr int SV_MAX_S = 8;
constexpr int SV_MAX_R = 3;
constexpr int SV_MAX_BAND = 4096;                   // (near + far) / step at most
constexpr double STEREO_ZNEAR = 0.01;               // as gaustar_amd.mesh_depth

struct StereoCamera {            // 152 bytes; gaustar_amd.stereo.CAMERA_DTYPE
    RigPinhole cam;              // the pose RELATIVE to the reference camera (R_sr, t_sr), the source's own fx, fy, cx, cy
    const void* image;           // sweep: the source's luma [H,W] uint8; consistency: its refined depth [H,W] f32
    const unsigned char* state;  // consistency: its state from the sweep [H,W]; the sweep does not read it
    int H, W;
};
static_assert(sizeof(StereoCamera) == 152 && offsetof(StereoCamera, image) == 128 && offsetof(StereoCamera, H) == 144,
              "StereoCamera is CAMERA_DTYPE's layout");

struct StereoParams {
    double step, near, far, background, min_var, min_score;
    int k_min, min_sources, keep;
};

// ---------------------------------------------------------------------------------------------------- luma
__host__ __device__ __forceinline__ unsigned luma_of(unsigned r, unsigned g, unsigned b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// n pixels; vec: rgb and out are 4-byte aligned (then so are a quad's 12 bytes in and 4 bytes out)
__global__ void __launch_bounds__(256) stereo_luma_kernel(int n, const unsigned char* __restrict__ rgb, unsigned char* __restrict__ out,
                                                          int vec)
{
    const int quads = (n + 3) >> 2;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < quads; q += gridDim.x * 256) {
        const int p = 4 * q;
        if (vec && p + 4 <= n) {
            const unsigned* in = reinterpret_cast<const unsigned*>(rgb + 3 * (size_t)p);
            const unsigned a = in[0], b = in[1], c = in[2];                       // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
            const unsigned y0 = luma_of(a & 255u, (a >> 8) & 255u, (a >> 16) & 255u);
            const unsigned y1 = luma_of(a >> 24, b & 255u, (b >> 8) & 255u);
            const unsigned y2 = luma_of((b >> 16) & 255u, b >> 24, c & 255u);
            const unsigned y3 = luma_of((c >> 8) & 255u, (c >> 16) & 255u, c >> 24);
            *reinterpret_cast<unsigned*>(out + p) = y0 | (y1 << 8) | (y2 << 16) | (y3 << 24);
        } else {
            for (int i = p; i < n && i < p + 4; ++i) out[i] = (unsigned char)luma_of(rgb[3 * (size_t)i], rgb[3 * (size_t)i + 1], rgb[3 * (size_t)i + 2]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- the sweep
// One warped tap: the reference pixel with the ray (qx, qy, 1) = ((c - cx) / fx, (r - cy) / fy, 1) (it may lie off the image, the
// formula does not care) on the plane at depth z, seen by the source -> the bilinear luma there, -1 where the warp is invalid.
__device__ __forceinline__ double warp_tap(const StereoCamera& sc, double qx, double qy, double z)
{
    const double Lx = qx * z, Ly = qy * z;
    double lx, ly, lz;
    rig_local(sc.cam.rc, Lx, Ly, z, lx, ly, lz);
    if (!(lz > STEREO_ZNEAR)) return -1.0;
    double u, v;
    rig_pixel(sc.cam.rc.fx, lx, lz, sc.cam.cx, u);
    rig_pixel(sc.cam.rc.fy, ly, lz, sc.cam.cy, v);
    // 0 <= floor(u) <= W - 2 and 0 <= floor(v) <= H - 2, tested in double: a NaN or a huge pixel is never converted
    if (!(u >= 0.0 && u < (double)(sc.W - 1) && v >= 0.0 && v < (double)(sc.H - 1))) return -1.0;
    const int x0 = (int)u, y0 = (int)v;
    const double ax = u - (double)x0, ay = v - (double)y0;
    const unsigned char* q = static_cast<const unsigned char*>(sc.image) + (size_t)y0 * sc.W + x0;
    const double i00 = (double)q[0], i01 = (double)q[1], i10 = (double)q[sc.W], i11 = (double)q[sc.W + 1];
    return (1.0 - ay) * ((1.0 - ax) * i00 + ax * i01) + ay * ((1.0 - ax) * i10 + ax * i11);
}

// grid (ceil(W / 16), ceil(H / 16)); dynamic LDS: (S + 1) (16 + 2 R)^2 doubles and 8 ints
template <int R>
__global__ void __launch_bounds__(SV_BLOCK) stereo_sweep_kernel(int H, int W, const unsigned char* __restrict__ luma,
                                                                const float* __restrict__ prior, double fx, double fy, double cx, double cy,
                                                                int S, const StereoCamera* __restrict__ src, StereoParams p,
                                                                float* __restrict__ depth, float* __restrict__ score,
                                                                unsigned char* __restrict__ state, short* __restrict__ plane)
{
    constexpr int K = 2 * R + 1, N = K * K, P = SV_TILE + 2 * R, PP = P * P;
    extern __shared__ __align__(16) unsigned char smem[];
    double* wp = reinterpret_cast<double*>(smem);        // [S][P][P]: the warped patches of the current plane
    double* gp = wp + S * PP;                            // [P][P]: the reference luma, 0 off the image
    int* red = reinterpret_cast<int*>(gp + PP);          // [8]: per wave the least k_lo and the largest k_hi

    const int t = threadIdx.x, tx = t & (SV_TILE - 1), ty = t >> 4;
    const int r0 = blockIdx.y * SV_TILE, c0 = blockIdx.x * SV_TILE;
    const int r = r0 + ty, c = c0 + tx;
    const bool in_img = r < H && c < W;
    const size_t at = (size_t)r * W + c;
    const float d32 = in_img ? prior[at] : 0.f;
    const double d = (double)d32;
    const bool covered = in_img && d > STEREO_ZNEAR && d < p.background;
    int k_lo = 1, k_hi = 0;
    if (covered) {      // (d + far) / step <= (background + far) / step, which the host has checked against int16
        const double lo = ceil((d - p.near) / p.step), hi = floor((d + p.far) / p.step);
        k_lo = lo > (double)p.k_min ? (int)lo : p.k_min;
        k_hi = (int)hi;
    }
    const bool banded = covered && k_lo <= k_hi;
    int mn = banded ? k_lo : INT_MAX, mx = banded ? k_hi : INT_MIN;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, __shfl_xor(mn, o, 64));
        mx = max(mx, __shfl_xor(mx, o, 64));
    }
    if ((t & 63) == 0) {
        red[t >> 6] = mn;
        red[4 + (t >> 6)] = mx;
    }
    for (int i = t; i < PP; i += SV_BLOCK) {
        const int py = i / P, px = i - py * P;
        const int rr = r0 - R + py, cc = c0 - R + px;
        gp[i] = (rr >= 0 && rr < H && cc >= 0 && cc < W) ? (double)luma[(size_t)rr * W + cc] : 0.0;
    }
    __syncthreads();
    const int tile_lo = min(min(red[0], red[1]), min(red[2], red[3])), tile_hi = max(max(red[4], red[5]), max(red[6], red[7]));

    // the reference window: integer sums; every tap on the image
    const double thr = (double)(N * N) * p.min_var;
    int A = 0, Vr = 0;
    bool active = false;
    if (tile_lo <= tile_hi && banded && r >= R && r + R < H && c >= R && c + R < W) {
        int B = 0;
#pragma unroll
        for (int dy = 0; dy < K; ++dy)
#pragma unroll
            for (int dx = 0; dx < K; ++dx) {
                const int g = (int)gp[(ty + dy) * P + tx + dx];
                A += g;
                B += g * g;
            }
        Vr = N * B - A * A;
        active = !((double)Vr < thr);
    }

    // the rays of the (at most two) patch taps this lane warps: they depend on neither the plane nor the source
    constexpr int TRIPS = (PP + SV_BLOCK - 1) / SV_BLOCK;
    double qx[TRIPS], qy[TRIPS];
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) {
        const int j = t + i * SV_BLOCK, py = j / P, px = j - py * P;
        qx[i] = ((double)(c0 - R + px) - cx) / fx;
        qy[i] = ((double)(r0 - R + py) - cy) / fy;
    }

    double best = -2.0, cm = 0.0, cp = 0.0, prev = 0.0;
    bool have = false, cm_ok = false, cp_ok = false, prev_ok = false;
    int kb = -1;
    for (int k = tile_lo; k <= tile_hi; ++k) {      // (an empty range where no pixel of the tile has a band: the tile leaves at once)
        const double z = (double)k * p.step;
        __syncthreads();                            // the previous plane's reads are done
        for (int s = 0; s < S; ++s) {
            const StereoCamera& sc = src[s];
#pragma unroll
            for (int i = 0; i < TRIPS; ++i) {
                const int j = t + i * SV_BLOCK;
                if (j < PP) wp[s * PP + j] = warp_tap(sc, qx[i], qy[i], z);
            }
        }
        __syncthreads();
        if (active && k >= k_lo && k <= k_hi) {
            double top[SV_MAX_S];
#pragma unroll
            for (int i = 0; i < SV_MAX_S; ++i) top[i] = -2.0;
            int v = 0;
            for (int s = 0; s < S; ++s) {
                const double* ws = wp + s * PP + ty * P + tx;
                const double* gs = gp + ty * P + tx;
                double Sw = 0.0, Sww = 0.0, Swg = 0.0;
                bool bad = false;
#pragma unroll 1
                for (int dy = 0; dy < K; ++dy)      // (a row of taps at a time: the whole window in flight takes 249 VGPRs at R = 3)
#pragma unroll
                    for (int dx = 0; dx < K; ++dx) {
                        const double w = ws[dy * P + dx], g = gs[dy * P + dx];
                        bad |= w < 0.0;
                        Sw += w;
                        Sww += w * w;
                        Swg += w * g;
                    }
                if (bad) continue;
                const double Vs = (double)N * Sww - Sw * Sw;
                if (!(Vs >= thr)) continue;
                double x = ((double)N * Swg - Sw * (double)A) / sqrt(Vs * (double)Vr);
                ++v;
#pragma unroll
                for (int i = 0; i < SV_MAX_S; ++i)
                    if (x > top[i]) {
                        const double y = top[i];
                        top[i] = x;
                        x = y;
                    }
            }
            const bool usable = v >= p.min_sources;
            double cost = 0.0;
            if (usable) {
                const int T = min(p.keep, v);
                cost = top[0];
#pragma unroll
                for (int i = 1; i < SV_MAX_S; ++i)
                    if (i < T) cost += top[i];
                cost = cost / (double)T;
                if (!have || cost > best) {
                    best = cost;
                    kb = k;
                    have = true;
                    cm = prev;
                    cm_ok = prev_ok;
                    cp_ok = false;
                } else if (k == kb + 1) {
                    cp = cost;
                    cp_ok = true;
                }
            }
            prev = cost;
            prev_ok = usable;
        }
    }

    if (!in_img) return;
    const int st = !covered ? 0 : (!have ? 1 : (best < p.min_score ? 2 : 3));
    float out_depth = d32;
    if (st == 3) {
        double delta = 0.0;
        if (cm_ok && cp_ok) {
            const double den = (cm - 2.0 * best) + cp;
            if (den < 0.0) {
                delta = (0.5 * (cm - cp)) / den;
                delta = delta < -0.5 ? -0.5 : (delta > 0.5 ? 0.5 : delta);
            }
        }
        out_depth = (float)(((double)kb + delta) * p.step);
    }
    // (the prior's bits, a NaN's payload included: moved as an integer)
    reinterpret_cast<unsigned*>(depth)[at] = st == 3 ? __float_as_uint(out_depth) : reinterpret_cast<const unsigned*>(prior)[at];
    score[at] = st >= 2 ? (float)best : -2.f;
    plane[at] = (short)(st >= 2 ? kb : -1);
    state[at] = (unsigned char)st;
}

// ---------------------------------------------------------------------------------------------------- consistency
__global__ void __launch_bounds__(256) stereo_consistency_kernel(int H, int W, const float* __restrict__ depth,
                                                                 const unsigned char* __restrict__ state, double fx, double fy, double cx,
                                                                 double cy, int S, const StereoCamera* __restrict__ src, double tol,
                                                                 int min_consistent, unsigned char* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * W) return;
    int st = state[i];
    if (st == 3) {
        const int r = i / W, c = i - r * W;
        const double z = (double)depth[i];
        const double Lx = (((double)c - cx) / fx) * z, Ly = (((double)r - cy) / fy) * z;
        int n = 0;
        for (int s = 0; s < S; ++s) {
            const StereoCamera& sc = src[s];
            double lx, ly, lz;
            rig_local(sc.cam.rc, Lx, Ly, z, lx, ly, lz);
            if (!(lz > STEREO_ZNEAR)) continue;
            double u, v;
            rig_pixel(sc.cam.rc.fx, lx, lz, sc.cam.cx, u);
            rig_pixel(sc.cam.rc.fy, ly, lz, sc.cam.cy, v);
            bool ok = true;
            const int col = rig_query(u, sc.W, ok), row = rig_query(v, sc.H, ok);
            if (!ok) continue;
            const size_t q = (size_t)row * sc.W + col;
            if (sc.state[q] < 3) continue;
            const double diff = (double)static_cast<const float*>(sc.image)[q] - lz;
            if (fabs(diff) <= tol) ++n;
        }
        if (n >= min_consistent) st = 4;
    }
    out[i] = (unsigned char)st;
}

// ---------------------------------------------------------------------------------------------------- merge
__device__ __forceinline__ float merge_voxel(float th, float wh, float ts, float ws, double min_weight)
{
    return ((double)ws >= min_weight && wh == 1.f && ts > th) ? ts : th;
}

__device__ __forceinline__ float4 merge_color(float4 c, float4 ws)
{
    return make_float4(ws.x > 0.f ? c.x : 0.f, ws.y > 0.f ? c.y : 0.f, ws.z > 0.f ? c.z : 0.f, ws.w > 0.f ? c.w : 0.f);
}

__global__ void __launch_bounds__(256) stereo_merge_kernel(FusionGrid g, const float* __restrict__ tsdf_h, const float* __restrict__ weight_h,
                                                           const float* __restrict__ tsdf_s, const float* __restrict__ weight_s,
                                                           const float* __restrict__ color_s, double min_weight, float* __restrict__ tsdf,
                                                           float* __restrict__ weight, float* __restrict__ color,
                                                           unsigned char* __restrict__ touched)
{
    const int unit = blockIdx.x;
    const int ux = unit % g.nu[0], uy = (unit / g.nu[0]) % g.nu[1], uz = unit / (g.nu[0] * g.nu[1]);
    const size_t nx = (size_t)g.nu[0] * FU, ny = (size_t)g.nu[1] * FU, nz = (size_t)g.nu[2] * FU;
    const size_t vol = nx * ny * nz;
    int any = 0;
    for (int q = threadIdx.x; q < FU_QUADS; q += 256) {
        const int x0 = (q & 3) * 4, y = (q >> 2) & (FU - 1), z = q >> 6;
        const size_t at = (((size_t)uz * FU + z) * ny + ((size_t)uy * FU + y)) * nx + (size_t)ux * FU + x0;
        const float4 TH = *reinterpret_cast<const float4*>(tsdf_h + at), WH = *reinterpret_cast<const float4*>(weight_h + at);
        const float4 TS = *reinterpret_cast<const float4*>(tsdf_s + at), WS = *reinterpret_cast<const float4*>(weight_s + at);
        float4 T;
        T.x = merge_voxel(TH.x, WH.x, TS.x, WS.x, min_weight);
        T.y = merge_voxel(TH.y, WH.y, TS.y, WS.y, min_weight);
        T.z = merge_voxel(TH.z, WH.z, TS.z, WS.z, min_weight);
        T.w = merge_voxel(TH.w, WH.w, TS.w, WS.w, min_weight);
        any |= (WH.x == 1.f && fabsf(T.x) < 1.f) || (WH.y == 1.f && fabsf(T.y) < 1.f) || (WH.z == 1.f && fabsf(T.z) < 1.f) ||
               (WH.w == 1.f && fabsf(T.w) < 1.f);
        *reinterpret_cast<float4*>(tsdf + at) = T;
        *reinterpret_cast<float4*>(weight + at) = WH;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            *reinterpret_cast<float4*>(color + ch * vol + at) = merge_color(*reinterpret_cast<const float4*>(color_s + ch * vol + at), WS);
    }
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) touched[unit] = any ? 1 : 0;
}

inline bool is_finite(double v) { return v - v == 0.0; }

// the host copy of a camera table, before anything is launched from its device copy
const char* stereo_cameras_error(int n, const StereoCamera* cams, bool consistency)
{
    for (int k = 0; k < n; ++k) {
        const StereoCamera& c = cams[k];
        const RigCamera& rc = c.cam.rc;
        for (int i = 0; i < 9; ++i)
            if (!is_finite(rc.R[i])) return "a camera is not finite";
        if (!is_finite(rc.t[0]) || !is_finite(rc.t[1]) || !is_finite(rc.t[2]) || !is_finite(c.cam.cx) || !is_finite(c.cam.cy)) return "a camera is not finite";
        if (!(rc.fx > 0.0) || !(rc.fy > 0.0) || !is_finite(rc.fx) || !is_finite(rc.fy)) return "focal lengths must be positive and finite";
        if (c.H < 2 || c.W < 2) return "a source image must be at least 2 x 2";
        if ((long long)c.H * c.W >= (1ll << 31)) return "a source image is too large";
        if (!c.image) return "a source image is null";
        if (consistency && (!c.state || (reinterpret_cast<uintptr_t>(c.image) & 3))) return "a source's state is null or its depth not 4-byte aligned";
    }
    return nullptr;
}

const char* stereo_reference_error(int H, int W, const double* ref_cam)
{
    if (H < 2 || W < 2) return "the image must be at least 2 x 2";
    if ((long long)H * W > (1ll << 31) - 256 || H > 16 * 65535) return "image too large";      // (a pixel index plus a workgroup fits an int)
    if (!ref_cam) return "required pointer is null";
    for (int i = 0; i < 4; ++i)
        if (!is_finite(ref_cam[i])) return "the reference camera is not finite";
    if (!(ref_cam[0] > 0.0) || !(ref_cam[1] > 0.0)) return "focal lengths must be positive and finite";
    return nullptr;
}

template <int R>
void launch_sweep(int H, int W, const unsigned char* luma, const float* prior, const double* rc, int S, const StereoCamera* src,
                  const StereoParams& p, float* depth, float* score, unsigned char* state, short* plane, hipStream_t st)
{
    constexpr int P = SV_TILE + 2 * R;
    const size_t lds = (size_t)(S + 1) * P * P * sizeof(double) + 8 * sizeof(int);
    stereo_sweep_kernel<R><<<dim3((W + SV_TILE - 1) / SV_TILE, (H + SV_TILE - 1) / SV_TILE), SV_BLOCK, lds, st>>>(
        H, W, luma, prior, rc[0], rc[1], rc[2], rc[3], S, src, p, depth, score, state, plane);
}

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

int gsr_stereo_camera_bytes(void) { return (int)sizeof(StereoCamera); }

int gsr_stereo_luma(int H, int W, const unsigned char* rgb, unsigned char* luma, gsr_stream_t stream)
{
    clear_error();
    if (H < 1 || W < 1) return fail_msg("gsr_stereo_luma: the image size must be positive");
    if ((long long)H * W * 3 >= (1ll << 31)) return fail_msg("gsr_stereo_luma: image too large");
    if (!rgb || !luma) return fail_msg("gsr_stereo_luma: required pointer is null");
    const int n = H * W, quads = (n + 3) >> 2;
    const int vec = ((reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(luma)) & 3) == 0;
    const int blocks = (quads + 255) / 256;
    stereo_luma_kernel<<<blocks < 2048 ? blocks : 2048, 256, 0, (hipStream_t)stream>>>(n, rgb, luma, vec);
    GSR_CHECK_LAUNCH("stereo_luma_kernel");
    return 0;
}

int gsr_stereo_sweep(int H, int W, const unsigned char* luma, const float* prior, const double* ref_cam, int n_sources,
                     const void* sources_host, const void* sources, const double* params, int radius, int min_sources, int keep,
                     float* depth, float* score, unsigned char* state, short* plane, gsr_stream_t stream)
{
    clear_error();
    if (const char* e = stereo_reference_error(H, W, ref_cam)) return fail_msg((std::string("gsr_stereo_sweep: ") + e).c_str());
    if (n_sources < 1 || n_sources > SV_MAX_S) return fail_msg("gsr_stereo_sweep: n_sources must be between 1 and 8");
    if (radius < 1 || radius > SV_MAX_R) return fail_msg("gsr_stereo_sweep: radius must be 1, 2 or 3");
    if (!params) return fail_msg("gsr_stereo_sweep: required pointer is null");
    StereoParams p;
    p.step = params[0], p.near = params[1], p.far = params[2], p.background = params[3], p.min_var = params[4], p.min_score = params[5];
    for (int i = 0; i < 6; ++i)
        if (!is_finite(params[i])) return fail_msg("gsr_stereo_sweep: a parameter is not finite");
    if (!(p.step > 0.0)) return fail_msg("gsr_stereo_sweep: step must be positive");
    if (p.near < 0.0 || p.far < 0.0) return fail_msg("gsr_stereo_sweep: near and far must not be negative");
    if (!((p.near + p.far) / p.step <= (double)SV_MAX_BAND)) return fail_msg("gsr_stereo_sweep: (near + far) / step must be at most 4096");
    if (!(p.background > STEREO_ZNEAR)) return fail_msg("gsr_stereo_sweep: background must be beyond znear");
    if (!((p.background + p.far) / p.step < 32768.0)) return fail_msg("gsr_stereo_sweep: the farthest plane index does not fit int16");
    if (!(p.min_var > 0.0)) return fail_msg("gsr_stereo_sweep: min_var must be positive");
    if (min_sources < 1 || min_sources > n_sources) return fail_msg("gsr_stereo_sweep: min_sources must be between 1 and n_sources");
    if (keep < 1 || keep > n_sources) return fail_msg("gsr_stereo_sweep: keep must be between 1 and n_sources");
    if (!luma || !prior || !sources_host || !sources || !depth || !score || !state || !plane)
        return fail_msg("gsr_stereo_sweep: required pointer is null");
    if ((reinterpret_cast<uintptr_t>(prior) | reinterpret_cast<uintptr_t>(depth) | reinterpret_cast<uintptr_t>(score)) & 3)
        return fail_msg("gsr_stereo_sweep: prior, depth and score must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(plane) & 1) return fail_msg("gsr_stereo_sweep: plane must be 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(sources) & 7) return fail_msg("gsr_stereo_sweep: the camera table must be 8-byte aligned");
    if (const char* e = stereo_cameras_error(n_sources, static_cast<const StereoCamera*>(sources_host), false))
        return fail_msg((std::string("gsr_stereo_sweep: ") + e).c_str());
    p.k_min = (int)floor(STEREO_ZNEAR / p.step) + 1;      // step >= (znear + far) / 32768: no overflow
    p.min_sources = min_sources;
    p.keep = keep;
    const StereoCamera* src = static_cast<const StereoCamera*>(sources);
    hipStream_t st = (hipStream_t)stream;
    if (radius == 1) launch_sweep<1>(H, W, luma, prior, ref_cam, n_sources, src, p, depth, score, state, plane, st);
    else if (radius == 2) launch_sweep<2>(H, W, luma, prior, ref_cam, n_sources, src, p, depth, score, state, plane, st);
    else launch_sweep<3>(H, W, luma, prior, ref_cam, n_sources, src, p, depth, score, state, plane, st);
    GSR_CHECK_LAUNCH("stereo_sweep_kernel");
    return 0;
}

int gsr_stereo_consistency(int H, int W, const float* depth, const unsigned char* state, const double* ref_cam, int n_sources,
                           const void* sources_host, const void* sources, double tol, int min_consistent, unsigned char* state_out,
                           gsr_stream_t stream)
{
    clear_error();
    if (const char* e = stereo_reference_error(H, W, ref_cam)) return fail_msg((std::string("gsr_stereo_consistency: ") + e).c_str());
    if (n_sources < 1 || n_sources > SV_MAX_S) return fail_msg("gsr_stereo_consistency: n_sources must be between 1 and 8");
    if (!(tol > 0.0) || !is_finite(tol)) return fail_msg("gsr_stereo_consistency: tol must be positive");
    if (min_consistent < 1 || min_consistent > n_sources) return fail_msg("gsr_stereo_consistency: min_consistent must be between 1 and n_sources");
    if (!depth || !state || !sources_host || !sources || !state_out) return fail_msg("gsr_stereo_consistency: required pointer is null");
    if (reinterpret_cast<uintptr_t>(depth) & 3) return fail_msg("gsr_stereo_consistency: depth must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(sources) & 7) return fail_msg("gsr_stereo_consistency: the camera table must be 8-byte aligned");
    if (const char* e = stereo_cameras_error(n_sources, static_cast<const StereoCamera*>(sources_host), true))
        return fail_msg((std::string("gsr_stereo_consistency: ") + e).c_str());
    stereo_consistency_kernel<<<(H * W + 255) / 256, 256, 0, (hipStream_t)stream>>>(
        H, W, depth, state, ref_cam[0], ref_cam[1], ref_cam[2], ref_cam[3], n_sources, static_cast<const StereoCamera*>(sources), tol,
        min_consistent, state_out);
    GSR_CHECK_LAUNCH("stereo_consistency_kernel");
    return 0;
}

int gsr_stereo_merge(const int* grid, const float* tsdf_h, const float* weight_h, const float* tsdf_s, const float* weight_s,
                     const float* color_s, double min_weight, float* tsdf, float* weight, float* color, unsigned char* touched,
                     gsr_stream_t stream)
{
    clear_error();
    if (const char* e = fusion_grid_error(grid)) return fail_msg((std::string("gsr_stereo_merge: ") + e).c_str());
    if (!(min_weight > 0.0) || !is_finite(min_weight)) return fail_msg("gsr_stereo_merge: min_weight must be positive");
    if (!tsdf_h || !weight_h || !tsdf_s || !weight_s || !color_s || !tsdf || !weight || !color || !touched)
        return fail_msg("gsr_stereo_merge: required pointer is null");
    if ((reinterpret_cast<uintptr_t>(tsdf_h) | reinterpret_cast<uintptr_t>(weight_h) | reinterpret_cast<uintptr_t>(tsdf_s) |
         reinterpret_cast<uintptr_t>(weight_s) | reinterpret_cast<uintptr_t>(color_s) | reinterpret_cast<uintptr_t>(tsdf) |
         reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(color)) & 15)
        return fail_msg("gsr_stereo_merge: the volumes' arrays must be 16-byte aligned");
    const FusionGrid g = fusion_grid(grid);
    stereo_merge_kernel<<<g.nu[0] * g.nu[1] * g.nu[2], 256, 0, (hipStream_t)stream>>>(g, tsdf_h, weight_h, tsdf_s, weight_s, color_s,
                                                                                     min_weight, tsdf, weight, color, touched);
    GSR_CHECK_LAUNCH("stereo_merge_kernel");
    return 0;
}

}  // extern "C"
