// gsr_meshdepth.hip -- the ground-truth depth map and mask of a frame's input mesh, per camera of the rig
// (data_process/render_depth_from_mesh.py:13-101, `render_mesh_depth_w_aitviewer`): the input of the depth and mask losses,
// of detect_topo_err and of warp_mesh_using_flow's visibility tests.  The reference renders them with an OpenGL renderer
// (aitviewer's HeadlessRenderer); here a depth-only triangle rasterizer draws one mesh for one pinhole camera per call and
// also returns the visible face per pixel.
//
// The rules (tests/meshdepth_ref.py restates them in numpy, operation by operation; everything is f64, contraction off):
//   camera    cam16 = gsr_rig.h's 14 doubles (R row-major, t, fx, fy) plus cx, cy.  local = R p + t,
//             x = fx * (lx / lz) + cx, y = fy * (ly / lz) + cy, in this operation order.
//   pixels    the centre of pixel (row r, column c) is at image coordinates (x, y) = (c, r): the convention of rig_project
//             followed by rig_query's int(pix + 0.5), so a vertex finds its own depth at the pixel it queries.  OpenGL
//             presumably samples at c + 0.5; parity with aitviewer is NOT pinned (neither is available to compare with).
//   skipped   a face with an index outside [0, V); a face with any vertex at lz <= znear (counted in n_clipped; a departure
//             from GL clipping: the cameras of a capture rig stand outside the subject); a face whose
//             area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0) is 0 or not finite.
//   coverage  E_i(c, r) = (x_k - x_j) * (r - y_j) - (y_k - y_j) * (c - x_j), (j, k) = (i + 1, i + 2) mod 3, the weight of
//             vertex i.  A pixel is covered iff all three E_i have the sign of `area` or are zero (inclusive edges, no
//             back-face culling).  Pixel range per axis: ceil(min) .. floor(max), clamped to the image IN DOUBLE before any
//             conversion to int; an empty range skips the face.  (A finite area implies six finite coordinates: an infinite
//             or NaN coordinate makes one of the two products infinite or NaN, and so the difference.)
//   depth     iz = (E_0 / area) / z_0 + (E_1 / area) / z_1 + (E_2 / area) / z_2, summed left to right;
//             z = (float)(1.0 / iz); the sample is kept iff z is finite and > 0.
//   winner    per pixel the smallest 64-bit key (bits(z) << 32) | face: the nearest depth, ties to the lower face index.
//   outputs   depth [H,W] f32 = z or `background`; mask [H,W] u8 = 255 / 0; face [H,W] i32 = the face or -1; n_clipped.
//
// Kernels (no float atomics, no scratch; the result is an integer minimum, so it does not depend on scheduling, on
// small_max or on the order of the big-face list):
//   key image            H W 64-bit words set to all ones (no valid key: z > 0 is finite, so bits(z) < 0x7f800000)
//   md_face_kernel       8 lanes per face: transform, skip rules, pixel range.  A range of at most small_max pixels is
//                        walked by the 8 lanes, a 64-bit atomicMin per covered pixel (one lane per face walks too many
//                        dependent steps: 81 920 faces fill a fifth of the device).  A larger one appends the face to
//                        the big-face list: up to
//                        MD_MID_MAX pixels at its front ("mid"), beyond that at its back ("huge"); a face is in one of the
//                        two, so both fit the F entries.
//   md_big_kernel        fixed grid, reads the two list lengths on the device.  A mid face is one work item: a wave walks
//                        the pixels of its range in row-major order, 64 at a time (at most MD_MID_MAX / 64 steps).  A huge
//                        face is 64 work items, one per interleaved row slice, one wave per item with its lanes across the
//                        columns: a face over the whole image is spread over the device.  Nothing is serial in a face's
//                        pixel count beyond max(small_max, MD_MID_MAX / 64) samples.
//   md_resolve_kernel    key image -> depth, mask, face; copies the clipped-face counter out.
// Both walks sample through md_sample on an MdFace that md_setup derived from the face index alone, so a pixel's key has
// the same bits whichever kernel produced it.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_rig.h"

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int MD_BLOCK = 256;
constexpr int MD_SLICES = 64;          // interleaved row slices of a huge face
constexpr int MD_MID_MAX = 4096;       // pixels in the range of a mid face: 64 steps of a wave
constexpr int MD_BIG_BLOCKS = 2048;    // md_big_kernel's fixed grid: 8 192 waves
// default of small_max: 32 steps of md_face_kernel's 8 lanes.  Config C's faces (ranges of up to 90 pixels) all stay below it:
// camera 0 takes 82 us at 64 and 50 us from 128 on (profiles/mesh_depth_config_c.txt); what a listed face costs is its
// append (md_face_kernel)
constexpr int MD_SMALL_MAX = 256;
constexpr int MD_FACE_LANES = 8;       // lanes of md_face_kernel per face
constexpr unsigned long long MD_EMPTY = ~0ull;

struct MdCounters {   // zeroed by the wrapper before md_face_kernel
    unsigned n_mid, n_huge;
    int n_clipped;
    unsigned pad;
};

struct MdFace {
    double x[3], y[3], z[3], area;
    int c_lo, c_hi, r_lo, r_hi;
};

enum { MD_SKIP = 0, MD_CLIPPED = 1, MD_DRAW = 2 };

__device__ __forceinline__ int md_setup(const RigPinhole& cam, int H, int W, int V, const double* __restrict__ verts,
                                        const int* __restrict__ faces, int f, double znear, MdFace& t)
{
    bool clipped = false;
    for (int k = 0; k < 3; ++k) {
        const int v = faces[3 * (size_t)f + k];
        if ((unsigned)v >= (unsigned)V) return MD_SKIP;
        const double* p = verts + 3 * (size_t)v;
        double lx, ly, lz;
        rig_local(cam.rc, p[0], p[1], p[2], lx, ly, lz);
        clipped = clipped || lz <= znear;
        rig_pixel(cam.rc.fx, lx, lz, cam.cx, t.x[k]);
        rig_pixel(cam.rc.fy, ly, lz, cam.cy, t.y[k]);
        t.z[k] = lz;
    }
    if (clipped) return MD_CLIPPED;
    t.area = (t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (t.y[1] - t.y[0]) * (t.x[2] - t.x[0]);
    if (t.area == 0.0 || !(fabs(t.area) < INFINITY)) return MD_SKIP;
    const double c_lo = fmax(ceil(fmin(fmin(t.x[0], t.x[1]), t.x[2])), 0.0);
    const double c_hi = fmin(floor(fmax(fmax(t.x[0], t.x[1]), t.x[2])), (double)(W - 1));
    const double r_lo = fmax(ceil(fmin(fmin(t.y[0], t.y[1]), t.y[2])), 0.0);
    const double r_hi = fmin(floor(fmax(fmax(t.y[0], t.y[1]), t.y[2])), (double)(H - 1));
    if (!(c_lo <= c_hi) || !(r_lo <= r_hi)) return MD_SKIP;
    t.c_lo = (int)c_lo;   // (all four in [0, W - 1] resp. [0, H - 1] here)
    t.c_hi = (int)c_hi;
    t.r_lo = (int)r_lo;
    t.r_hi = (int)r_hi;
    return MD_DRAW;
}

// the key of face f at pixel (r, c), or MD_EMPTY where the face does not cover it or the sample is not kept
__device__ __forceinline__ unsigned long long md_sample(const MdFace& t, int f, int r, int c)
{
    const double pc = (double)c, pr = (double)r;
    const double e0 = (t.x[2] - t.x[1]) * (pr - t.y[1]) - (t.y[2] - t.y[1]) * (pc - t.x[1]);
    const double e1 = (t.x[0] - t.x[2]) * (pr - t.y[2]) - (t.y[0] - t.y[2]) * (pc - t.x[2]);
    const double e2 = (t.x[1] - t.x[0]) * (pr - t.y[0]) - (t.y[1] - t.y[0]) * (pc - t.x[0]);
    const bool in = t.area > 0.0 ? (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) : (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
    if (!in) return MD_EMPTY;
    const double iz = (e0 / t.area) / t.z[0] + (e1 / t.area) / t.z[1] + (e2 / t.area) / t.z[2];
    const float z = (float)(1.0 / iz);
    if (!(z > 0.f && z < INFINITY)) return MD_EMPTY;
    return ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)f;
}

// PEEK: a plain load first drops a sample that already loses (keys only fall, so it loses for good).  md_big_kernel's lanes
// peek; in md_face_kernel's serial walks the load's latency would sit on every step (config C's rig: 56.3 us per camera with,
// 48.1 us without, tools/bench_mesh_depth.py at small_max = 64).
template <bool PEEK>
__device__ __forceinline__ void md_put(unsigned long long* __restrict__ keys, size_t i, unsigned long long key)
{
    if (!PEEK || key < keys[i]) atomicMin(keys + i, key);
}

// MD_FACE_LANES neighbouring lanes per face: each derives the face (the loads coalesce) and walks every MD_FACE_LANES-th pixel
// of its range in row-major order
__global__ void __launch_bounds__(MD_BLOCK) md_face_kernel(int H, int W, int V, int F, const double* __restrict__ verts,
                                                           const int* __restrict__ faces, RigPinhole cam, double znear, int small_max,
                                                           unsigned long long* __restrict__ keys, MdCounters* __restrict__ cnt,
                                                           int* __restrict__ big)
{
    const long long tid = (long long)blockIdx.x * MD_BLOCK + threadIdx.x;
    const int f = (int)(tid / MD_FACE_LANES), sub = (int)(tid % MD_FACE_LANES);
    MdFace t;
    const int what = f < F ? md_setup(cam, H, W, V, verts, faces, f, znear, t) : MD_SKIP;
    const unsigned long long clipped = __ballot(what == MD_CLIPPED && sub == 0);
    if (clipped && (threadIdx.x & 63) == 0) atomicAdd(&cnt->n_clipped, (int)__popcll(clipped));
    if (what != MD_DRAW) return;
    const int nx = t.c_hi - t.c_lo + 1;
    const long long n = (long long)nx * (t.r_hi - t.r_lo + 1);
    if (n > small_max) {
        if (sub != 0) return;
        // A face is appended once, to one end: front + back <= F entries.  The counter is one word, and a word takes some 88
        // atomic instructions per us whatever their lanes: with every face of config C listed (small_max = 8) the call grows
        // by 14.6 us per lane of MD_FACE_LANES, that is per 1 280 waves (150 / 208 / 325 / 558 us at 4 / 8 / 16 / 32 lanes).  At
        // the default small_max none of them is listed, and an image has room for few faces above it.
        if (n <= MD_MID_MAX) big[atomicAdd(&cnt->n_mid, 1u)] = f;
        else big[F - 1 - (int)atomicAdd(&cnt->n_huge, 1u)] = f;
        return;
    }
    for (long long p = sub; p < n; p += MD_FACE_LANES) {
        const int r = t.r_lo + (int)(p / nx), c = t.c_lo + (int)(p % nx);
        const unsigned long long key = md_sample(t, f, r, c);
        if (key != MD_EMPTY) md_put<false>(keys, (size_t)r * W + c, key);
    }
}

__global__ void __launch_bounds__(MD_BLOCK) md_big_kernel(int H, int W, int V, int F, const double* __restrict__ verts,
                                                          const int* __restrict__ faces, RigPinhole cam, double znear,
                                                          unsigned long long* __restrict__ keys, const MdCounters* __restrict__ cnt,
                                                          const int* __restrict__ big)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * MD_BLOCK + threadIdx.x) >> 6;
    const long long waves = (long long)gridDim.x * (MD_BLOCK / 64);
    const long long huge_items = (long long)cnt->n_huge * MD_SLICES, items = huge_items + cnt->n_mid;
    for (long long it = wave; it < items; it += waves) {   // (the huge faces first: they take the longest)
        const bool huge = it < huge_items;
        const int f = huge ? big[F - 1 - (int)(it / MD_SLICES)] : big[it - huge_items];
        MdFace t;
        if (md_setup(cam, H, W, V, verts, faces, f, znear, t) != MD_DRAW) continue;   // (never: the list holds drawn faces)
        if (huge) {
            for (int r = t.r_lo + (int)(it % MD_SLICES); r <= t.r_hi; r += MD_SLICES)
                for (int c = t.c_lo + lane; c <= t.c_hi; c += 64) {
                    const unsigned long long key = md_sample(t, f, r, c);
                    if (key != MD_EMPTY) md_put<true>(keys, (size_t)r * W + c, key);
                }
        } else {
            const int nx = t.c_hi - t.c_lo + 1, n = nx * (t.r_hi - t.r_lo + 1);   // (n <= MD_MID_MAX)
            for (int p = lane; p < n; p += 64) {
                const int r = t.r_lo + p / nx, c = t.c_lo + p % nx;
                const unsigned long long key = md_sample(t, f, r, c);
                if (key != MD_EMPTY) md_put<true>(keys, (size_t)r * W + c, key);
            }
        }
    }
}

__device__ __forceinline__ void md_resolve_one(unsigned long long key, float background, float& d, unsigned char& m, int& f)
{
    const bool hit = key != MD_EMPTY;
    d = hit ? __uint_as_float((unsigned)(key >> 32)) : background;
    m = hit ? 255 : 0;
    f = hit ? (int)(unsigned)key : -1;
}

// four pixels per lane where VEC (every output 16-byte resp. 4-byte aligned), the n % 4 pixels at the end one by one
template <bool VEC>
__global__ void __launch_bounds__(MD_BLOCK) md_resolve_kernel(int n, const unsigned long long* __restrict__ keys, float background,
                                                              const MdCounters* __restrict__ cnt, float* __restrict__ depth,
                                                              unsigned char* __restrict__ mask, int* __restrict__ face,
                                                              int* __restrict__ n_clipped)
{
    const int i = blockIdx.x * MD_BLOCK + threadIdx.x;
    if (i == 0) *n_clipped = cnt->n_clipped;
    if (VEC) {
        const int q = n / 4;
        if (i < q) {
            const ulonglong2 a = reinterpret_cast<const ulonglong2*>(keys)[2 * (size_t)i];
            const ulonglong2 b = reinterpret_cast<const ulonglong2*>(keys)[2 * (size_t)i + 1];
            float4 d;
            uchar4 m;
            int4 f;
            md_resolve_one(a.x, background, d.x, m.x, f.x);
            md_resolve_one(a.y, background, d.y, m.y, f.y);
            md_resolve_one(b.x, background, d.z, m.z, f.z);
            md_resolve_one(b.y, background, d.w, m.w, f.w);
            reinterpret_cast<float4*>(depth)[i] = d;
            reinterpret_cast<uchar4*>(mask)[i] = m;
            if (face) reinterpret_cast<int4*>(face)[i] = f;
        } else if (i < q + n % 4) {
            const int j = 4 * q + (i - q);
            int f;
            md_resolve_one(keys[j], background, depth[j], mask[j], f);
            if (face) face[j] = f;
        }
    } else if (i < n) {
        int f;
        md_resolve_one(keys[i], background, depth[i], mask[i], f);
        if (face) face[i] = f;
    }
}

inline size_t md_keys_bytes(int H, int W) { return sizeof(unsigned long long) * (size_t)H * (size_t)W; }

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

size_t gsr_mesh_depth_workspace_bytes(int H, int W, int F)
{
    if (H <= 0 || W <= 0 || F < 0) return 0;
    return md_keys_bytes(H, W) + sizeof(MdCounters) + sizeof(int) * (size_t)F;
}

int gsr_mesh_depth_view(int H, int W, int V, int F, const double* verts, const int* faces, const double* cam16, double znear,
                        float background, int small_max, void* workspace, float* depth, unsigned char* mask, int* face_or_null,
                        int* n_clipped, gsr_stream_t stream)
{
    clear_error();
    if (H <= 0 || W <= 0 || V < 0 || F < 0) return fail_msg("gsr_mesh_depth_view: sizes must be positive");
    if ((long long)H * W >= (1ll << 31)) return fail_msg("gsr_mesh_depth_view: image too large");
    if (!(fabsf(background) < INFINITY)) return fail_msg("gsr_mesh_depth_view: background must be finite");
    if (!cam16 || !workspace || !depth || !mask || !n_clipped || (F > 0 && (!faces || (V > 0 && !verts))))
        return fail_msg("gsr_mesh_depth_view: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    const int n = H * W;
    unsigned long long* keys = static_cast<unsigned long long*>(workspace);
    MdCounters* cnt = reinterpret_cast<MdCounters*>(static_cast<char*>(workspace) + md_keys_bytes(H, W));
    int* big = reinterpret_cast<int*>(cnt + 1);
    RigPinhole cam;
    cam.rc = rig_camera(cam16);
    cam.cx = cam16[14];
    cam.cy = cam16[15];
    GSR_CHECK(hipMemsetAsync(keys, 0xff, md_keys_bytes(H, W), st));
    GSR_CHECK(hipMemsetAsync(cnt, 0, sizeof(MdCounters), st));
    if (F > 0) {
        md_face_kernel<<<(unsigned)(((long long)F * MD_FACE_LANES + MD_BLOCK - 1) / MD_BLOCK), MD_BLOCK, 0, st>>>(H, W, V, F, verts, faces, cam, znear,
                                                                         small_max > 0 ? small_max : MD_SMALL_MAX, keys, cnt, big);
        md_big_kernel<<<MD_BIG_BLOCKS, MD_BLOCK, 0, st>>>(H, W, V, F, verts, faces, cam, znear, keys, cnt, big);
    }
    const bool vec = ((uintptr_t)workspace | (uintptr_t)depth | (uintptr_t)face_or_null) % 16 == 0 && (uintptr_t)mask % 4 == 0;
    if (vec)
        md_resolve_kernel<true><<<(n / 4 + 3 + MD_BLOCK - 1) / MD_BLOCK, MD_BLOCK, 0, st>>>(n, keys, background, cnt, depth, mask,
                                                                                           face_or_null, n_clipped);
    else
        md_resolve_kernel<false><<<(n + MD_BLOCK - 1) / MD_BLOCK, MD_BLOCK, 0, st>>>(n, keys, background, cnt, depth, mask,
                                                                                     face_or_null, n_clipped);
    GSR_CHECK_LAUNCH("mesh depth kernels");
    return 0;
}

}  // extern "C"
