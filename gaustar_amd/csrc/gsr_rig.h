// gsr_rig.h -- what the per-camera passes of a rig share (gsr_topo.hip: detect_topo_err, gsr_warp.hip: warp_mesh_using_flow;
// the camera alone also gsr_prep.hip, gsr_meshdepth.hip, gsr_hull.hip): the camera and its f64 projection, query_at_image's
// index, the depth-edge statistic get_depth_edge(depth, 2 R + 1) and the two image passes that reduce a depth map to the
// maxima it is normalised by, and the ping-pong loop of the Jacobi sweeps.
//
// Floating point follows the numpy restatements (tests/topo_ref.py, tests/warp_ref.py) operation by operation, so contraction
// into FMAs is off.  The pragma stands HERE because clang fixes the contraction mode where a function or template is defined,
// not where it is instantiated.
#pragma once
#include "gsr_internal.h"

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int RIG_BLOCK = 256;
constexpr int RIG_PARTS = 2048;   // workgroups of an image pass per map (grid-stride), = partials per statistic and map

struct RigCamera {
    double R[9], t[3];   // COLMAP world-to-camera rotation (row-major) and translation (cmr["extrinsics"][c][:3])
    double fx, fy;       // cmr["intrinsics"][c][0,0], [1,1]
};

// the [host] camera block of the ABI: R (9, row-major), t (3), fx, fy
inline RigCamera rig_camera(const double* cam14)
{
    RigCamera cam;
    for (int i = 0; i < 9; ++i) cam.R[i] = cam14[i];
    for (int i = 0; i < 3; ++i) cam.t[i] = cam14[9 + i];
    cam.fx = cam14[12];
    cam.fy = cam14[13];
    return cam;
}

// with the principal point in pixels: gsr_mesh_depth_view's [host] block and a HullCamera's head (_rig.camera_block's 16 doubles)
struct RigPinhole {
    RigCamera rc;
    double cx, cy;
};

// local = R p + t, each row as ((R0 x + R1 y) + R2 z) + t
__host__ __device__ __forceinline__ void rig_local(const RigCamera& cam, double px, double py, double pz, double& lx, double& ly, double& lz)
{
    lx = ((cam.R[0] * px + cam.R[1] * py) + cam.R[2] * pz) + cam.t[0];
    ly = ((cam.R[3] * px + cam.R[4] * py) + cam.R[5] * pz) + cam.t[1];
    lz = ((cam.R[6] * px + cam.R[7] * py) + cam.R[8] * pz) + cam.t[2];
}

// one pixel coordinate of a local point: the quotient, then the product, then the sum.  (Not returned by value: clang then
// takes the pixel for well defined and hull_carve_kernel's bounds test comes out with two operands exchanged.)
__host__ __device__ __forceinline__ void rig_pixel(double f, double l, double lz, double c, double& pix) { pix = f * (l / lz) + c; }

// warp_mesh.py:47-74 in double: local = R p + t, row = fy y / z + H / 2, col = fx x / z + W / 2 (no principal point).  The
// pixel is the un-rounded one: query_at_image adds its 0.5 itself (rig_query)
__device__ __forceinline__ void rig_project(const RigCamera& cam, int H, int W, double px, double py, double pz, double& lx,
                                            double& ly, double& lz, double& pr, double& pc)
{
    rig_local(cam, px, py, pz, lx, ly, lz);
    rig_pixel(cam.fy, ly, lz, H * 0.5, pr);
    rig_pixel(cam.fx, lx, lz, W * 0.5, pc);
}

// query_at_image's index (warp_mesh.py:106-117): np.int32(pix + 0.5) truncates toward zero, NaN and values out of the int32
// range become INT_MIN (x86's conversion); the index is clipped to [0, n - 1] and the lookup valid iff clipping changed nothing.
// The returned index is always in [0, n - 1], so a caller may read first and test `ok` later.
// The detection used to spell the rule as a range test, y = pix + 0.5 in (-1, n) with index (int)y.  That is this predicate
// (n >= 1): for y inside the int32 range p = trunc(y), and 0 <= trunc(y) <= n - 1 holds exactly for -1 < y < n (trunc maps
// (-1, 0] to 0 and [k, k + 1) to k); a y outside the int32 range is <= -2^31 - 1 < -1 or >= 2^31 > n and gives INT_MIN < 0,
// invalid under both; NaN fails every comparison, so it fails the range test and gives INT_MIN here.  Where valid both read
// index (int)y.  No double outside the int range is ever converted.
__device__ __forceinline__ int rig_query(double pix, int n, bool& ok)
{
    const double y = pix + 0.5;
    const int p = (y > -2147483649.0 && y < 2147483648.0) ? (int)y : INT_MIN;
    const int c = min(max(p, 0), n - 1);
    ok = ok && p == c;
    return c;
}

// cv2 BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba), for any offset
__device__ __forceinline__ int reflect101(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

// get_depth_edge(depth, 2 R + 1) at (y, x): d = min(depth, m), var = max(blur(d^2) - blur(d)^2, 0) with cv2.blur's normalised
// (2 R + 1)^2 box filter.  OpenCV documents the box filter of f32 data as a running sum in double, scaled by the reciprocal of
// the window size and rounded to f32 on output; that claim has not been checked against cv2 here (cv2 is not available).
// The values are summed row by row in double, then the rows.  While the non-zero values of a window (d, and likewise d^2) lie
// within a factor of 2^23 of each other that sum is exact, so the order of the running sum does not matter: every value is a
// multiple of the smallest one's f32 ulp, and N of them sum to less than N 2^(23 + 24) ulps, which a double holds exactly up
// to N = 2^6 -- the 49 of R = 3; the 9 of R = 1 would leave room for a factor of 2^25.  d^2 is squared in f32 (numpy
// `depth ** 2`), blur(d) is squared in f32.
template <int R>
__device__ __forceinline__ float edge_var(const float* __restrict__ g, int H, int W, int y, int x, float m)
{
    constexpr int K = 2 * R + 1;
    double s1 = 0.0, s2 = 0.0;
    int xs[K];
#pragma unroll
    for (int k = 0; k < K; ++k) xs[k] = reflect101(x + k - R, W);
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
        const float* row = g + (size_t)reflect101(y + dy, H) * W;
        double r1 = 0.0, r2 = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float d = fminf(row[xs[k]], m);
            r1 += (double)d;
            r2 += (double)(d * d);
        }
        s1 += r1;
        s2 += r2;
    }
    const float mean = (float)(s1 * (1.0 / (K * K))), sq_mean = (float)(s2 * (1.0 / (K * K)));
    return fmaxf(sq_mean - mean * mean, 0.f);
}

// max over the RIG_PARTS partials at `p`, by the whole workgroup (every lane gets it); red: RIG_BLOCK floats of LDS
__device__ float block_max_of_parts(const float* __restrict__ p, float* red)
{
    float v = -INFINITY;
    for (int i = threadIdx.x; i < RIG_PARTS; i += RIG_BLOCK) v = fmaxf(v, p[i]);
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = RIG_BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__device__ void block_store_max(float v, float* red, float* out)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = RIG_BLOCK / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

// m = f32(1.1 * max(depth[depth < max_depth])) (warp_mesh.py:122-124: np.float32 max times a Python float, in double as
// NumPy 1.x evaluates it); -inf when no pixel is below max_depth
__device__ __forceinline__ float clip_depth(float dmax) { return dmax == -INFINITY ? -INFINITY : (float)((double)dmax * 1.1); }

// The two image passes of a camera with n_maps depth maps, on a grid of RIG_PARTS workgroups per map.  Partials of map `map`:
// its depth maximum at parts[map RIG_PARTS ..], its var maximum at parts[(n_maps + map) RIG_PARTS ..].  Each consumer reduces
// the partials it needs itself (a fixed-size max: order-free, so the result does not depend on which workgroup ran first), and
// the var pass and the per-vertex lookup compute `var` with the same edge_var, so edge_vis agrees bit for bit between the
// maximum and the lookup.  H W < 2^31 (checked at the ABI), but a pixel index plus the grid stride may not fit an int: the
// depth pass counts in 64 bits, the var pass, which divides the index, in an unsigned.
__device__ __forceinline__ void depth_max_pass(int n, const float* __restrict__ g, float max_depth, int map,
                                               float* __restrict__ parts)
{
    __shared__ float red[RIG_BLOCK];
    float v = -INFINITY;
    for (long long i = blockIdx.x * RIG_BLOCK + threadIdx.x; i < n; i += RIG_PARTS * RIG_BLOCK) {
        const float d = g[i];
        if (d < max_depth) v = fmaxf(v, d);
    }
    block_store_max(v, red, parts + map * RIG_PARTS + blockIdx.x);
}

template <int R>
__device__ __forceinline__ void var_max_pass(int H, int W, const float* __restrict__ g, int map, int n_maps,
                                             float* __restrict__ parts)
{
    __shared__ float red[RIG_BLOCK];
    const float m = clip_depth(block_max_of_parts(parts + map * RIG_PARTS, red));
    float v = 0.f;
    if (m != -INFINITY)
        for (unsigned i = blockIdx.x * RIG_BLOCK + threadIdx.x; i < (unsigned)(H * W); i += RIG_PARTS * RIG_BLOCK)
            v = fmaxf(v, edge_var<R>(g, H, W, (int)(i / W), (int)(i % W), m));
    block_store_max(v, red, parts + (n_maps + map) * RIG_PARTS + blockIdx.x);
}

// `sweeps` Jacobi sweeps from `in`, alternating between `out` and `tmp`: sweep s writes buffer k = (sweeps - 1 - s) % 2 of
// {out, tmp}, so the last one lands in `out`.  launch(src, dst, k) enqueues one sweep.
template <class T, class Launch>
inline void ping_pong_sweeps(int sweeps, const T* in, T* out, T* tmp, Launch launch)
{
    T* b[2] = {out, tmp};
    const T* src = in;
    for (int s = 0; s < sweeps; ++s) {
        const int k = (sweeps - 1 - s) & 1;
        launch(src, b[k], k);
        src = b[k];
    }
}

}  // namespace

}  // namespace gsr
