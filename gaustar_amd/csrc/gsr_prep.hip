// gsr_prep.hip -- what a sequence needs before frame 0 (data_process/ahq2gaustar.py): the rectified images
// (:50-81 `img_translate`, `rgb_convert`; gaustar_tools/cmr_convert.py:71-109, :214-223 `img_convert`: cv2.undistort followed
// by the translation) and the colours of the first mesh's vertices (:124-160 `compute_mesh_color`).
//
// The rules (tests/prep_ref.py restates them in numpy, operation by operation; everything is f64, contraction off):
//
// gsr_image_rectify, for output pixel (row r, column c), everything in double:
//   Plain path, taken iff dist5 is null or all five coefficients are exactly 0:
//     su = c + (cx - 0.5 W), sv = r + (cy - 0.5 H).
//     This is img_translate's dst(c) = src(c + dx).
//   Distorted path:
//     x = (c - 0.5 W) / fx, y = (r - 0.5 H) / fy, r2 = x x + y y.
//     rad = 1 + r2 (k1 + r2 (k2 + r2 k3)).
//     xd = x rad + (2 p1 x y + p2 (r2 + 2 x x)).
//     yd = y rad + (p1 (r2 + 2 y y) + 2 p2 x y).
//     su = fx xd + cx, sv = fy yd + cy.
//   Bilinear sampling:
//     x0 = floor(su), ax = su - x0, likewise y0, ay.
//     The four taps are src where inside the image and border[ch] where outside (cv2's BORDER_CONSTANT).
//     If su or sv is not finite or outside the int range, the pixel is border.
//     Value = (t00 (1 - ax) + t01 ax) (1 - ay) + (t10 (1 - ax) + t11 ax) ay.
//     Stored as (uint8) rint(value), half to even.
//   (Products are formed left to right: 2 p1 x y = ((2 p1) x) y.  "Outside the int range": su resp. sv is not in
//   [-2^31, 2^31 - 1), so that x0 and x0 + 1 are ints; such a pixel has no tap inside an image of H W < 2^31 pixels.)
//
// gsr_mesh_color_view, per vertex (ahq2gaustar.py:141-151): rig_project (no principal point), row and column by rig_query,
//   visible = valid && fabs(lz - (double)depth[row, col]) < threshold (NaN compares false; no test on the sign of lz: the
//   depth map decides).  A visible vertex adds its pixel's three bytes and 1 to its record (r, g, b, n) of four int32.
//
// gsr_mesh_color_finish, per vertex with sums (S_r, S_g, S_b, n):
//   mean = S / (double)n (NaN where n = 0, numpy's 0 / 0 at :158); rgb = (2 S + n) / (2 n) in 64-bit integers (the mean
//   rounded half up); filled_at = 0 where n > 0.  Then `fill_sweeps` Jacobi sweeps s = 1, 2, ...: a vertex without a colour
//   after sweep s - 1 that has k > 0 neighbours with one takes, per channel, (2 S + k) / (2 k) of those neighbours' rgb
//   (S: their sum) and filled_at = s; a sweep reads only the previous sweep's state.  A vertex still without a colour gets
//   default_color and filled_at = 255.  counters[0] = vertices with n = 0, counters[1] = vertices that got default_color.
//
// Kernels (no float atomics, no scratch, integers for everything that is accumulated):
//   prep_rectify_kernel<C, DIST, VEC>   VEC: a lane computes four consecutive pixels (of the flat [H W] order) and stores their
//                                       4 C bytes as C whole dwords; taken when dst is 4-byte aligned.  The H W % 4 pixels
//                                       at the end, and every pixel of an unaligned dst, are stored byte by byte.  Taps are
//                                       byte loads: neighbouring lanes read neighbouring texels, and a tap's row is shared
//                                       by the next output row, so they come from the caches.
//   prep_color_view_kernel              one lane per vertex, four 32-bit integer atomicAdd where it is visible.  Cameras on
//                                       other streams add to the same records: integer adds commute, so the sums do not
//                                       depend on which camera ran first.
//   prep_finish_init / _sweep / _final  one lane per vertex.  The state of the sweeps is one word per vertex,
//                                       r | g << 8 | b << 16 | filled_at << 24 with 255 = no colour yet, so a neighbour costs
//                                       one load; the sweeps alternate between two buffers (ping_pong_sweeps).
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_rig.h"

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int PREP_BLOCK = 256;
constexpr int PREP_MAX_BLOCKS = 4096;   // grid cap of the image kernel (grid-stride beyond it)
constexpr unsigned PREP_NONE = 255u;    // filled_at of a vertex without a colour

struct RectParams {
    double fx, fy, cx, cy;
    double k1, k2, p1, p2, k3;
    unsigned char border[4];
};

// the source position (su, sv) of output pixel (r, c)
template <bool DIST>
__device__ __forceinline__ void rect_source(const RectParams& p, int H, int W, int r, int c, double& su, double& sv)
{
    if (!DIST) {
        su = (double)c + (p.cx - 0.5 * (double)W);
        sv = (double)r + (p.cy - 0.5 * (double)H);
    } else {
        const double x = ((double)c - 0.5 * (double)W) / p.fx;
        const double y = ((double)r - 0.5 * (double)H) / p.fy;
        const double r2 = x * x + y * y;
        const double rad = 1.0 + r2 * (p.k1 + r2 * (p.k2 + r2 * p.k3));
        const double xd = x * rad + (2.0 * p.p1 * x * y + p.p2 * (r2 + 2.0 * x * x));
        const double yd = y * rad + (p.p1 * (r2 + 2.0 * y * y) + 2.0 * p.p2 * x * y);
        su = p.fx * xd + p.cx;
        sv = p.fy * yd + p.cy;
    }
}

// the C bytes of output pixel `pix` (< H W)
template <int C, bool DIST>
__device__ __forceinline__ void rect_pixel(const RectParams& p, int H, int W, const unsigned char* __restrict__ src, int pix,
                                           unsigned char* out)
{
    const int r = pix / W, c = pix - r * W;
    double su, sv;
    rect_source<DIST>(p, H, W, r, c, su, sv);
    // (NaN fails both comparisons; +-inf one of them).  A pixel that is not `ok` is computed at (0, 0) with every tap outside:
    // ax = ay = 0 there, so its value is (b 1 + b 0) 1 + (b 1 + b 0) 0 = b exactly.  Nothing below branches, so a lane's 4 C
    // loads -- 16 C with four pixels -- can be issued together and waited for once
    const bool ok = su >= -2147483648.0 && su < 2147483647.0 && sv >= -2147483648.0 && sv < 2147483647.0;
    su = ok ? su : 0.0;
    sv = ok ? sv : 0.0;
    const double fx0 = floor(su), fy0 = floor(sv);
    const double ax = su - fx0, ay = sv - fy0;
    const int x0 = (int)fx0, y0 = (int)fy0;   // (both < 2^31 - 1: x0 + 1, y0 + 1 are ints)
    const bool inx0 = ok && (unsigned)x0 < (unsigned)W, inx1 = ok && (unsigned)(x0 + 1) < (unsigned)W;
    const bool iny0 = (unsigned)y0 < (unsigned)H, iny1 = (unsigned)(y0 + 1) < (unsigned)H;
    // every tap is LOADED from a coordinate clamped into the image (always a valid address) and USED only where it is inside
    const unsigned char* row0 = src + ((size_t)min(max(y0, 0), H - 1) * W) * C;
    const unsigned char* row1 = src + ((size_t)min(max(y0 + 1, 0), H - 1) * W) * C;
    const size_t o0 = (size_t)min(max(x0, 0), W - 1) * C, o1 = (size_t)min(max(x0 + 1, 0), W - 1) * C;
    const double bx = 1.0 - ax, by = 1.0 - ay;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const double b = (double)p.border[ch];
        const unsigned char l00 = row0[o0 + ch], l01 = row0[o1 + ch], l10 = row1[o0 + ch], l11 = row1[o1 + ch];
        const double t00 = (iny0 && inx0) ? (double)l00 : b;
        const double t01 = (iny0 && inx1) ? (double)l01 : b;
        const double t10 = (iny1 && inx0) ? (double)l10 : b;
        const double t11 = (iny1 && inx1) ? (double)l11 : b;
        const double v = (t00 * bx + t01 * ax) * by + (t10 * bx + t11 * ax) * ay;
        out[ch] = (unsigned char)rint(v);   // (v in [0, 255]: a blend of bytes with weights in [0, 1])
    }
}

template <int C, bool DIST, bool VEC>
__global__ void __launch_bounds__(PREP_BLOCK) prep_rectify_kernel(int H, int W, const unsigned char* __restrict__ src,
                                                                  unsigned char* __restrict__ dst, RectParams p)
{
    const int n = H * W;
    const long long tid = (long long)blockIdx.x * PREP_BLOCK + threadIdx.x, stride = (long long)gridDim.x * PREP_BLOCK;
    if (VEC) {
        const int q = n / 4;
        for (long long g = tid; g < q; g += stride) {
            unsigned char b[4 * C];
#pragma unroll
            for (int k = 0; k < 4; ++k) rect_pixel<C, DIST>(p, H, W, src, (int)(4 * g + k), b + k * C);
            unsigned* o = reinterpret_cast<unsigned*>(dst + (size_t)g * (4 * C));
#pragma unroll
            for (int w = 0; w < C; ++w)
                o[w] = (unsigned)b[4 * w] | ((unsigned)b[4 * w + 1] << 8) | ((unsigned)b[4 * w + 2] << 16) | ((unsigned)b[4 * w + 3] << 24);
        }
        if (tid < n - 4 * q) {   // the H W % 4 pixels at the end
            const int pix = 4 * q + (int)tid;
            unsigned char b[C];
            rect_pixel<C, DIST>(p, H, W, src, pix, b);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) dst[(size_t)pix * C + ch] = b[ch];
        }
    } else {
        for (long long i = tid; i < n; i += stride) {
            unsigned char b[C];
            rect_pixel<C, DIST>(p, H, W, src, (int)i, b);
#pragma unroll
            for (int ch = 0; ch < C; ++ch) dst[(size_t)i * C + ch] = b[ch];
        }
    }
}

template <int C>
void launch_rectify(int H, int W, const unsigned char* src, unsigned char* dst, const RectParams& p, bool dist, hipStream_t st)
{
    const bool vec = (uintptr_t)dst % 4 == 0;
    const long long items = vec ? ((long long)H * W + 3) / 4 : (long long)H * W;   // (>= the H W % 4 lanes of the tail)
    long long blocks = (items + PREP_BLOCK - 1) / PREP_BLOCK;
    if (blocks > PREP_MAX_BLOCKS) blocks = PREP_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    const unsigned g = (unsigned)blocks;
    if (dist) {
        if (vec) prep_rectify_kernel<C, true, true><<<g, PREP_BLOCK, 0, st>>>(H, W, src, dst, p);
        else prep_rectify_kernel<C, true, false><<<g, PREP_BLOCK, 0, st>>>(H, W, src, dst, p);
    } else {
        if (vec) prep_rectify_kernel<C, false, true><<<g, PREP_BLOCK, 0, st>>>(H, W, src, dst, p);
        else prep_rectify_kernel<C, false, false><<<g, PREP_BLOCK, 0, st>>>(H, W, src, dst, p);
    }
}

__global__ void __launch_bounds__(PREP_BLOCK) prep_color_view_kernel(int H, int W, int V, const double* __restrict__ verts,
                                                                     const unsigned char* __restrict__ image,
                                                                     const float* __restrict__ depth, RigCamera cam, double threshold,
                                                                     int* __restrict__ sums)
{
    const int v = blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (v >= V) return;
    const double* p = verts + 3 * (size_t)v;
    double lx, ly, lz, pr, pc;
    rig_project(cam, H, W, p[0], p[1], p[2], lx, ly, lz, pr, pc);
    bool ok = true;
    const int row = rig_query(pr, H, ok), col = rig_query(pc, W, ok);   // (both in range whatever `ok`)
    const size_t pix = (size_t)row * W + col;
    const bool visible = ok && fabs(lz - (double)depth[pix]) < threshold;
    if (!visible) return;
    const unsigned char* px = image + 3 * pix;
    int* s = sums + 4 * (size_t)v;
    atomicAdd(s + 0, (int)px[0]);
    atomicAdd(s + 1, (int)px[1]);
    atomicAdd(s + 2, (int)px[2]);
    atomicAdd(s + 3, 1);
}

// one atomicAdd per wave of the lanes whose `flag` is set (every lane of the workgroup calls it)
__device__ __forceinline__ void prep_count(bool flag, int* counter)
{
    const unsigned long long m = __ballot(flag);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(counter, (int)__popcll(m));
}

__global__ void __launch_bounds__(PREP_BLOCK) prep_finish_init_kernel(int V, const int* __restrict__ sums, double* __restrict__ mean,
                                                                      unsigned* __restrict__ state, int* __restrict__ counters)
{
    const int v = blockIdx.x * PREP_BLOCK + threadIdx.x;
    const bool live = v < V;
    bool unseen = false;
    if (live) {
        const int4 s = reinterpret_cast<const int4*>(sums)[v];
        const double n = (double)s.w;
        mean[3 * (size_t)v + 0] = (double)s.x / n;
        mean[3 * (size_t)v + 1] = (double)s.y / n;
        mean[3 * (size_t)v + 2] = (double)s.z / n;
        unsigned word = PREP_NONE << 24;
        if (s.w > 0) {
            const long long n2 = 2ll * s.w;
            const unsigned r = (unsigned)((2ll * s.x + s.w) / n2), g = (unsigned)((2ll * s.y + s.w) / n2), b = (unsigned)((2ll * s.z + s.w) / n2);
            word = (r & 255u) | ((g & 255u) << 8) | ((b & 255u) << 16);
        } else {
            unseen = true;
        }
        state[v] = word;
    }
    prep_count(unseen, counters);
}

__global__ void __launch_bounds__(PREP_BLOCK) prep_finish_sweep_kernel(int V, const int* __restrict__ off, const int* __restrict__ nbr,
                                                                       unsigned sweep, const unsigned* __restrict__ src,
                                                                       unsigned* __restrict__ dst)
{
    const int v = blockIdx.x * PREP_BLOCK + threadIdx.x;
    if (v >= V) return;
    unsigned word = src[v];
    if ((word >> 24) == PREP_NONE) {
        long long sr = 0, sg = 0, sb = 0, k = 0;
        for (int e = off[v]; e < off[v + 1]; ++e) {
            const int j = nbr[e];
            if ((unsigned)j >= (unsigned)V) continue;
            const unsigned w = src[j];
            if ((w >> 24) == PREP_NONE) continue;
            sr += w & 255u;
            sg += (w >> 8) & 255u;
            sb += (w >> 16) & 255u;
            ++k;
        }
        if (k > 0)
            word = (unsigned)((2 * sr + k) / (2 * k)) | ((unsigned)((2 * sg + k) / (2 * k)) << 8) | ((unsigned)((2 * sb + k) / (2 * k)) << 16) |
                   (sweep << 24);
    }
    dst[v] = word;
}

__global__ void __launch_bounds__(PREP_BLOCK) prep_finish_final_kernel(int V, const unsigned* __restrict__ state, unsigned fallback,
                                                                       unsigned char* __restrict__ rgb, unsigned char* __restrict__ filled_at,
                                                                       int* __restrict__ counters)
{
    const int v = blockIdx.x * PREP_BLOCK + threadIdx.x;
    const bool live = v < V;
    bool unfilled = false;
    if (live) {
        unsigned word = state[v];
        unfilled = (word >> 24) == PREP_NONE;
        if (unfilled) word = fallback | (PREP_NONE << 24);
        rgb[3 * (size_t)v + 0] = (unsigned char)(word & 255u);
        rgb[3 * (size_t)v + 1] = (unsigned char)((word >> 8) & 255u);
        rgb[3 * (size_t)v + 2] = (unsigned char)((word >> 16) & 255u);
        filled_at[v] = (unsigned char)(word >> 24);
    }
    prep_count(unfilled, counters + 1);
}

inline unsigned pblocks(long long n) { return (unsigned)((n + PREP_BLOCK - 1) / PREP_BLOCK); }

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

int gsr_image_rectify(int H, int W, int C, const unsigned char* src, unsigned char* dst, const double* cam4,
                      const double* dist5_or_null, const unsigned char* border, gsr_stream_t stream)
{
    clear_error();
    if (H <= 0 || W <= 0) return fail_msg("gsr_image_rectify: sizes must be positive");
    if (C != 1 && C != 3 && C != 4) return fail_msg("gsr_image_rectify: C must be 1, 3 or 4");
    if ((long long)H * W >= (1ll << 31)) return fail_msg("gsr_image_rectify: image too large");
    if (!src || !dst || !cam4 || !border) return fail_msg("gsr_image_rectify: required pointer is null");
    if (src == dst) return fail_msg("gsr_image_rectify: dst must not be src");
    RectParams p;
    p.fx = cam4[0];
    p.fy = cam4[1];
    p.cx = cam4[2];
    p.cy = cam4[3];
    bool dist = false;
    p.k1 = p.k2 = p.p1 = p.p2 = p.k3 = 0.0;
    if (dist5_or_null) {
        for (int i = 0; i < 5; ++i) dist = dist || dist5_or_null[i] != 0.0;   // (a NaN coefficient takes the distorted path)
        p.k1 = dist5_or_null[0];
        p.k2 = dist5_or_null[1];
        p.p1 = dist5_or_null[2];
        p.p2 = dist5_or_null[3];
        p.k3 = dist5_or_null[4];
    }
    for (int ch = 0; ch < 4; ++ch) p.border[ch] = ch < C ? border[ch] : 0;
    hipStream_t st = (hipStream_t)stream;
    if (C == 1) launch_rectify<1>(H, W, src, dst, p, dist, st);
    else if (C == 3) launch_rectify<3>(H, W, src, dst, p, dist, st);
    else launch_rectify<4>(H, W, src, dst, p, dist, st);
    GSR_CHECK_LAUNCH("prep_rectify_kernel");
    return 0;
}

int gsr_mesh_color_view(int H, int W, int V, const double* verts, const unsigned char* image, const float* depth,
                        const double* cam14, double threshold, int* sums, gsr_stream_t stream)
{
    clear_error();
    if (H <= 0 || W <= 0 || V < 0) return fail_msg("gsr_mesh_color_view: sizes must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail_msg("gsr_mesh_color_view: image too large");
    if (V == 0) return 0;
    if (!verts || !image || !depth || !cam14 || !sums) return fail_msg("gsr_mesh_color_view: required pointer is null");
    prep_color_view_kernel<<<pblocks(V), PREP_BLOCK, 0, (hipStream_t)stream>>>(H, W, V, verts, image, depth, rig_camera(cam14), threshold,
                                                                                sums);
    GSR_CHECK_LAUNCH("prep_color_view_kernel");
    return 0;
}

size_t gsr_mesh_color_workspace_bytes(int V) { return V <= 0 ? 0 : 3 * sizeof(unsigned) * (size_t)V; }

int gsr_mesh_color_finish(int V, const int* sums, const int* nbr_offsets, const int* nbr, int fill_sweeps,
                          const unsigned char* default_color, void* workspace, double* mean, unsigned char* rgb,
                          unsigned char* filled_at, int* counters, gsr_stream_t stream)
{
    clear_error();
    if (V < 0) return fail_msg("gsr_mesh_color_finish: negative size");
    if (fill_sweeps < 0 || fill_sweeps > 254) return fail_msg("gsr_mesh_color_finish: fill_sweeps must lie in 0..254");
    if (V == 0) return 0;
    if (!sums || !default_color || !workspace || !mean || !rgb || !filled_at || !counters ||
        (fill_sweeps > 0 && (!nbr_offsets || !nbr)))
        return fail_msg("gsr_mesh_color_finish: required pointer is null");
    if ((uintptr_t)sums % 16 != 0 || (uintptr_t)workspace % 4 != 0)
        return fail_msg("gsr_mesh_color_finish: sums must be 16-byte aligned, workspace 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned* first = static_cast<unsigned*>(workspace);
    unsigned *out = first + V, *tmp = first + 2 * (size_t)V;
    GSR_CHECK(hipMemsetAsync(counters, 0, 2 * sizeof(int), st));
    prep_finish_init_kernel<<<pblocks(V), PREP_BLOCK, 0, st>>>(V, sums, mean, first, counters);
    unsigned sweep = 0;
    ping_pong_sweeps(fill_sweeps, (const unsigned*)first, out, tmp, [&](const unsigned* src, unsigned* dst, int) {
        prep_finish_sweep_kernel<<<pblocks(V), PREP_BLOCK, 0, st>>>(V, nbr_offsets, nbr, ++sweep, src, dst);
    });
    const unsigned fallback = (unsigned)default_color[0] | ((unsigned)default_color[1] << 8) | ((unsigned)default_color[2] << 16);
    prep_finish_final_kernel<<<pblocks(V), PREP_BLOCK, 0, st>>>(V, fill_sweeps > 0 ? out : first, fallback, rgb, filled_at, counters);
    GSR_CHECK_LAUNCH("prep finish kernels");
    return 0;
}

}  // extern "C"
