// gsr_edit.hip -- editing a tracked sequence: the per-Gaussian passes of gaustar_tools/internal_use_tools/gstar_edit.py, which
// the reference runs on the host in numpy / trimesh / cv2 with its paths written into the file.  Here, over device tensors:
//   rigid fit's sums    edit_fit_centroid_kernel   per frame n, sum a, sum b over the anchors whose six coordinates are finite
//                       edit_fit_cross_kernel      H = sum (a - abar)(b - bbar)^T about those centroids (best_fit_transform, :48-54)
//                       edit_fit_finish_kernel     the [T,16] doubles the host's SVD reads (:55-64 stay on the host: a 3 x 3 per frame)
//   moving a model      edit_transform_kernel      (R0 x + R1 y) + R2 z [+ t] per coordinate, f64 from f32, rounded once (:146)
//                       edit_rotate_sh_kernel      the SH coefficients above the dc turned with the object (the reference leaves
//                                                  them fixed in the world): 64 Gaussians' rows staged through LDS, 16 bytes a lane
//   selecting           edit_halfspaces_kernel     OR over groups of AND over planes on the face centres (:81-102, as data)
//   cutting             edit_gather_kernel         the G rows per kept face of up to 8 parameter arrays in one launch (:114-116)
//   painting            edit_paint_kernel          edit_gs_color's loop over the anchor triangles, one lane per Gaussian (:316-385)
// The fit, the transform, the selection and the geometry of the paint are float64 without contraction, every operation in the
// order include/gsr.h states; the colour arithmetic of the paint is float32 without contraction, as the reference's.  No float
// atomics, no scratch: the fit's sums go through gsr_reduce.h's fixed-order reduction (two calls give the same bits), the
// paint's counters are integer atomics.  The point type, point_to_bary and bary_to_point are gsr_surface.h's.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_surface.h"
#include "gsr_reduce.h"

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int ED_BLOCK = MESH_BLOCK;
static_assert(ED_BLOCK == RED_BLOCK, "the fit's element passes use gsr_reduce.h's workgroup");

// ---------------------------------------------------------------- rigid fit: the sums
constexpr int FIT_GROUPS = 5;       // groups of RED_STRIDE partials per workgroup: {n, sum a}, {sum b}, H's three rows

// workspace [T][FIT_GROUPS][n_wg][RED_STRIDE] doubles
__device__ __forceinline__ double* fit_group(double* __restrict__ ws, int n_wg, int t, int g)
{
    return ws + ((size_t)t * FIT_GROUPS + g) * (size_t)n_wg * RED_STRIDE;
}

// anchor k of frame t: (a, b) = (src[k], dst[t, k]); false when one of the six coordinates is not finite (a lost point)
__device__ __forceinline__ bool fit_pair(int K, int t, int k, const double* __restrict__ src, const double* __restrict__ dst, D3& a, D3& b)
{
    a = load3(src, (size_t)k);
    b = load3(dst, (size_t)t * K + k);
    return finite3(a) && finite3(b);
}

// grid (n_wg, T)
__global__ void __launch_bounds__(ED_BLOCK) edit_fit_centroid_kernel(int K, const double* __restrict__ src, const double* __restrict__ dst,
                                                                     double* __restrict__ ws)
{
    const int t = blockIdx.y, n_wg = gridDim.x;
    double s4[4] = {0., 0., 0., 0.}, s3[3] = {0., 0., 0.};
    for (int k = blockIdx.x * ED_BLOCK + threadIdx.x; k < K; k += n_wg * ED_BLOCK) {
        D3 a, b;
        if (fit_pair(K, t, k, src, dst, a, b)) {
            s4[0] += 1.0; s4[1] += a.x; s4[2] += a.y; s4[3] += a.z;
            s3[0] += b.x; s3[1] += b.y; s3[2] += b.z;
        }
    }
    block_partials<4>(s4, fit_group(ws, n_wg, t, 0));
    block_partials<3>(s3, fit_group(ws, n_wg, t, 1));
}

// (n, abar, bbar) of frame t from the first pass's partials, in every thread; the whole workgroup calls this.  n == 0 gives
// NaN centroids.
__device__ __forceinline__ void fit_centroids(double* __restrict__ ws, int n_wg, int t, double& n, D3& abar, D3& bbar)
{
    __shared__ double c[7];
    double t4[4], t3[3];
    tree_total<4>(n_wg, fit_group(ws, n_wg, t, 0), t4);
    tree_total<3>(n_wg, fit_group(ws, n_wg, t, 1), t3);
    if (threadIdx.x == 0) {
        c[0] = t4[0];
        c[1] = t4[1] / t4[0]; c[2] = t4[2] / t4[0]; c[3] = t4[3] / t4[0];
        c[4] = t3[0] / t4[0]; c[5] = t3[1] / t4[0]; c[6] = t3[2] / t4[0];
    }
    __syncthreads();
    n = c[0];
    abar = {c[1], c[2], c[3]};
    bbar = {c[4], c[5], c[6]};
}

// grid (n_wg, T): H[i][j] = sum_k (a_i - abar_i)(b_j - bbar_j), each term one rounded product of two rounded differences
__global__ void __launch_bounds__(ED_BLOCK) edit_fit_cross_kernel(int K, const double* __restrict__ src, const double* __restrict__ dst,
                                                                  double* __restrict__ ws)
{
    const int t = blockIdx.y, n_wg = gridDim.x;
    double n;
    D3 abar, bbar;
    fit_centroids(ws, n_wg, t, n, abar, bbar);
    double h0[3] = {0., 0., 0.}, h1[3] = {0., 0., 0.}, h2[3] = {0., 0., 0.};
    for (int k = blockIdx.x * ED_BLOCK + threadIdx.x; k < K; k += n_wg * ED_BLOCK) {
        D3 a, b;
        if (fit_pair(K, t, k, src, dst, a, b)) {
            const D3 da = sub3(a, abar), db = sub3(b, bbar);
            h0[0] += da.x * db.x; h0[1] += da.x * db.y; h0[2] += da.x * db.z;
            h1[0] += da.y * db.x; h1[1] += da.y * db.y; h1[2] += da.y * db.z;
            h2[0] += da.z * db.x; h2[1] += da.z * db.y; h2[2] += da.z * db.z;
        }
    }
    block_partials<3>(h0, fit_group(ws, n_wg, t, 2));
    __syncthreads();                                         // (the three calls share one LDS array)
    block_partials<3>(h1, fit_group(ws, n_wg, t, 3));
    __syncthreads();
    block_partials<3>(h2, fit_group(ws, n_wg, t, 4));
}

// grid T: out[t] = {n, abar (3), bbar (3), H row-major (9)}
__global__ void __launch_bounds__(ED_BLOCK) edit_fit_finish_kernel(int n_wg, double* __restrict__ ws, double* __restrict__ out)
{
    const int t = blockIdx.x;
    double n;
    D3 abar, bbar;
    fit_centroids(ws, n_wg, t, n, abar, bbar);
    double* o = out + 16 * (size_t)t;
    if (threadIdx.x == 0) {
        o[0] = n;
        o[1] = abar.x; o[2] = abar.y; o[3] = abar.z;
        o[4] = bbar.x; o[5] = bbar.y; o[6] = bbar.z;
    }
    for (int r = 0; r < 3; ++r) {
        double h[3];
        __syncthreads();                                     // (tree_total<3>'s LDS array is read to its end)
        tree_total<3>(n_wg, fit_group(ws, n_wg, t, 2 + r), h);
        if (threadIdx.x == 0) { o[7 + 3 * r] = h[0]; o[8 + 3 * r] = h[1]; o[9 + 3 * r] = h[2]; }
    }
}

// ---------------------------------------------------------------- moving a model
struct Rigid { double r[9]; double t[3]; };

// rows of `stride` floats; columns [offset, offset + 3) of row i, in place
__global__ void __launch_bounds__(ED_BLOCK) edit_transform_kernel(long long n, int stride, int offset, float* __restrict__ x, Rigid m,
                                                                  int translate)
{
    const long long i = (long long)blockIdx.x * ED_BLOCK + threadIdx.x;
    if (i >= n) return;
    float* p = x + (size_t)i * stride + offset;
    const double px = p[0], py = p[1], pz = p[2];
    double o0 = (m.r[0] * px + m.r[1] * py) + m.r[2] * pz;
    double o1 = (m.r[3] * px + m.r[4] * py) + m.r[5] * pz;
    double o2 = (m.r[6] * px + m.r[7] * py) + m.r[8] * pz;
    if (translate) { o0 += m.t[0]; o1 += m.t[1]; o2 += m.t[2]; }
    p[0] = (float)o0; p[1] = (float)o1; p[2] = (float)o2;
}

constexpr int SH_GAUSS = 64;        // Gaussians per workgroup: 64 rows of 36, 96 or 180 bytes are a whole number of 16-byte pieces
constexpr int SH_BLOCK = 192;       // wave c takes channel c of the 64 Gaussians

// rest [N, M - 1, 3] f32 with M = L L; D [M,M] f64 row-major, block diagonal.  A workgroup's 64 rows are contiguous: they come
// in and go out 16 bytes a lane, whatever a row's own alignment, and turn in place in LDS (lane (g, c) reads and writes the
// same 15 words).  in == out is allowed.
template <int L>
__global__ void __launch_bounds__(SH_BLOCK) edit_rotate_sh_kernel(int N, const double* __restrict__ D, const float* in, float* out)
{
    constexpr int M = L * L, RW = 3 * (M - 1);
    __shared__ __attribute__((aligned(16))) float rows[SH_GAUSS * RW];
    __shared__ double d[M * M];
    const size_t base = (size_t)blockIdx.x * SH_GAUSS;
    const int ng = N - base < (size_t)SH_GAUSS ? (int)(N - base) : SH_GAUSS;
    const int nf = ng * RW;
    const float* src = in + base * RW;
    float* dst = out + base * RW;
    for (int e = threadIdx.x; e < M * M; e += SH_BLOCK) d[e] = D[e];
    for (int q = threadIdx.x; q < nf / 4; q += SH_BLOCK) reinterpret_cast<float4*>(rows)[q] = reinterpret_cast<const float4*>(src)[q];
    for (int e = (nf & ~3) + threadIdx.x; e < nf; e += SH_BLOCK) rows[e] = src[e];
    __syncthreads();
    const int c = threadIdx.x >> 6, g = threadIdx.x & 63;
    if (g < ng) {
        float* r = rows + g * RW + c;
        double x[M - 1];
#pragma unroll
        for (int k = 0; k < M - 1; ++k) x[k] = (double)r[3 * k];
#pragma unroll
        for (int l = 1; l < L; ++l) {
            const int o = l * l, w = 2 * l + 1;              // band l: coefficients [o, o + w) of the M, [o - 1, ...) of the rest
#pragma unroll
            for (int i = 0; i < w; ++i) {
                double s = d[(o + i) * M + o] * x[o - 1];
#pragma unroll
                for (int k = 1; k < w; ++k) s += d[(o + i) * M + o + k] * x[o - 1 + k];
                r[3 * (o - 1 + i)] = (float)s;
            }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nf / 4; q += SH_BLOCK) reinterpret_cast<float4*>(dst)[q] = reinterpret_cast<const float4*>(rows)[q];
    for (int e = (nf & ~3) + threadIdx.x; e < nf; e += SH_BLOCK) dst[e] = rows[e];
}

// ---------------------------------------------------------------- selecting and cutting
constexpr int HS_MAX_GROUPS = 16, HS_MAX_PLANES = 64;
struct HalfSpaces { double p[HS_MAX_PLANES][4]; int start[HS_MAX_GROUPS + 1]; int n_groups; };

// mask [F] uint8 = 1 iff for some group every plane has (a cx + b cy) + c cz + d > 0 at the face's centre ((v0 + v1) + v2) / 3
__global__ void __launch_bounds__(ED_BLOCK) edit_halfspaces_kernel(int F, int V, const int* __restrict__ faces, const float* __restrict__ verts,
                                                                   HalfSpaces hs, unsigned char* __restrict__ mask, int* __restrict__ err)
{
    const int f = blockIdx.x * ED_BLOCK + threadIdx.x;
    if (f >= F) return;
    int v[3];
    if (!mesh_face(faces, f, V, v)) { atomicOr(err, MESH_ERR_INDEX); mask[f] = 0; return; }
    double c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
        c[a] = (((double)verts[3 * (size_t)v[0] + a] + (double)verts[3 * (size_t)v[1] + a]) + (double)verts[3 * (size_t)v[2] + a]) / 3.0;
    bool any = false;
    for (int g = 0; g < hs.n_groups; ++g) {
        bool all = true;
        for (int j = hs.start[g]; j < hs.start[g + 1]; ++j)
            all = all && ((hs.p[j][0] * c[0] + hs.p[j][1] * c[1]) + hs.p[j][2] * c[2]) + hs.p[j][3] > 0.;
        any = any || all;
    }
    mask[f] = any;
}

constexpr int GR_MAX = 8;
// table e holds n_faces rows of words[e] 32-bit words (a face's G Gaussians are contiguous) and takes workgroups
// [first[e], first[e + 1]) of the launch
struct GatherTable { const unsigned* src[GR_MAX]; unsigned* dst[GR_MAX]; int words[GR_MAX]; unsigned first[GR_MAX + 1]; int n; };

// dst_e[j] = src_e[kept[j]] for every table e and new face j; an entry of kept outside [0, F) sets err and gives zeros
__global__ void __launch_bounds__(ED_BLOCK) edit_gather_kernel(int n_faces, int F, const int* __restrict__ kept, GatherTable tb,
                                                               int* __restrict__ err)
{
    int e = 0;
    while (e + 1 < tb.n && blockIdx.x >= tb.first[e + 1]) ++e;           // (uniform in the workgroup)
    const int w = tb.words[e];
    const long long i = (long long)(blockIdx.x - tb.first[e]) * ED_BLOCK + threadIdx.x;
    if (i >= (long long)n_faces * w) return;
    const int j = (int)(i / w), rem = (int)(i % w);
    const int f = kept[j];
    unsigned word = 0;
    if ((unsigned)f >= (unsigned)F) atomicOr(err, MESH_ERR_INDEX);
    else word = tb.src[e][(size_t)f * w + rem];
    tb.dst[e][i] = word;
}

// ---------------------------------------------------------------- painting
constexpr int PT_MAX_TRI = 64;
constexpr int PT_ROW = 18;          // a triangle in LDS: t0, t1, t2 (9), its corners' (u, v) (6), its normal (3)
constexpr float PT_C0 = 0.28209479177387814f;
struct PaintArgs {
    int N, G, F, V, n_tri, h, w, C, mode, shrink, alpha_min;
    float shrink_scale;
    double slack, max_dist;
};

__device__ __forceinline__ void wave_count(bool mine, int* __restrict__ word)
{
    const unsigned long long m = __ballot(mine);
    if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(word, __popcll(m));
}

// tri [n_tri,15] f64: a triangle's three anchors and their (u, v).  stats (zero before): n_painted, n_outside, n_inside[n_tri].
// scales [N,2] and dc [N,3] in place; a Gaussian no triangle touches keeps its bits.
__global__ void __launch_bounds__(ED_BLOCK) edit_paint_kernel(PaintArgs a, const int* __restrict__ faces, const float* __restrict__ verts,
                                                              const float* __restrict__ bary, const double* __restrict__ tri,
                                                              const unsigned char* __restrict__ tex, float* __restrict__ scales,
                                                              float* __restrict__ dc, int* __restrict__ stats, int* __restrict__ err)
{
    __shared__ double T[PT_MAX_TRI][PT_ROW];
    for (int e = threadIdx.x; e < a.n_tri * 15; e += ED_BLOCK) T[e / 15][e % 15] = tri[e];
    __syncthreads();
    if ((int)threadIdx.x < a.n_tri) {                        // n = -cross(t1 - t0, t2 - t1) / sqrt((x x + y y) + z z)
        double* r = T[threadIdx.x];
        const D3 t0 = {r[0], r[1], r[2]}, t1 = {r[3], r[4], r[5]}, t2 = {r[6], r[7], r[8]};
        const D3 cr = cross3(sub3(t1, t0), sub3(t2, t1));
        const double len = sqrt((cr.x * cr.x + cr.y * cr.y) + cr.z * cr.z);
        r[15] = -cr.x / len; r[16] = -cr.y / len; r[17] = -cr.z / len;
    }
    __syncthreads();

    const long long i = (long long)blockIdx.x * ED_BLOCK + threadIdx.x;
    bool live = i < a.N;
    D3 p = {0., 0., 0.};
    if (live) {
        const int f = (int)(i / a.G), g = (int)(i % a.G);
        int v[3];
        if ((unsigned)f >= (unsigned)a.F || !mesh_face(faces, f, a.V, v)) { atomicOr(err, MESH_ERR_INDEX); live = false; }
        else {
            const double b0 = bary[3 * g], b1 = bary[3 * g + 1], b2 = bary[3 * g + 2];
            const float *v0 = verts + 3 * (size_t)v[0], *v1 = verts + 3 * (size_t)v[1], *v2 = verts + 3 * (size_t)v[2];
            p = {(b0 * (double)v0[0] + b1 * (double)v1[0]) + b2 * (double)v2[0], (b0 * (double)v0[1] + b1 * (double)v1[1]) + b2 * (double)v2[1],
                 (b0 * (double)v0[2] + b1 * (double)v1[2]) + b2 * (double)v2[2]};
        }
    }
    float r = 0.f, gch = 0.f, b = 0.f;                       // the colour, formed from dc by the first triangle that paints
    bool have = false, shrunk = false;
    int outside = 0;
    for (int t = 0; t < a.n_tri; ++t) {
        const double* q = T[t];
        bool in = false;
        D3 nb = {0., 0., 0.};
        if (live) {
            const D3 t0 = {q[0], q[1], q[2]}, t1 = {q[3], q[4], q[5]}, t2 = {q[6], q[7], q[8]}, n = {q[15], q[16], q[17]};
            nb = point_to_bary(t0, t1, t2, p);
            const double dist = dot3(sub3(t0, p), n);
            in = nb.x >= -a.slack && nb.y >= -a.slack && nb.z >= -a.slack && -a.max_dist < dist && dist < a.max_dist;
        }
        wave_count(in, stats + 2 + t);
        if (!in) continue;
        shrunk = true;
        const double u = (nb.x * q[9] + nb.y * q[11]) + nb.z * q[13], v = (nb.x * q[10] + nb.y * q[12]) + nb.z * q[14];
        const double row = trunc(u * (double)a.h), col = trunc(v * (double)a.w);
        if (!(row >= 0. && row < (double)a.h && col >= 0. && col < (double)a.w)) { ++outside; continue; }
        const unsigned char* px = tex + ((size_t)(int)row * a.w + (int)col) * a.C;
        if (a.mode == 1 && a.C == 4 && !((int)px[3] > a.alpha_min)) continue;
        if (!have) {
            r = dc[3 * i] * PT_C0 + 0.5f; gch = dc[3 * i + 1] * PT_C0 + 0.5f; b = dc[3 * i + 2] * PT_C0 + 0.5f;
            have = true;
        }
        if (a.mode == 0) {
            const float k = (float)((double)px[0] / 255.0);
            r *= k; gch *= k; b *= k;
        } else {
            r = (float)((double)px[0] / 255.0); gch = (float)((double)px[1] / 255.0); b = (float)((double)px[2] / 255.0);
        }
    }
    wave_count(have, stats);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) outside += __shfl_down(outside, o, 64);
    if ((threadIdx.x & 63) == 0 && outside) atomicAdd(stats + 1, outside);
    if (shrunk && a.shrink) { scales[2 * i] = a.shrink_scale; scales[2 * i + 1] = a.shrink_scale; }
    if (have) { dc[3 * i] = (r - 0.5f) / PT_C0; dc[3 * i + 1] = (gch - 0.5f) / PT_C0; dc[3 * i + 2] = (b - 0.5f) / PT_C0; }
}

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

size_t gsr_edit_fit_workspace_bytes(int T, int K)
{
    if (T <= 0 || K <= 0) return 256;
    return align_up(sizeof(double) * RED_STRIDE * FIT_GROUPS * (size_t)T * (size_t)reduce_workgroups(K)) + 256;
}

int gsr_edit_fit_sums(int T, int K, const double* src, const double* dst, void* workspace, double* out, int* err, gsr_stream_t stream)
{
    (void)err;
    clear_error();
    if (T < 0 || K < 0) return fail_msg("gsr_edit_fit_sums: negative size");
    if (T > 65535) return fail_msg("gsr_edit_fit_sums: more than 65535 frames in one call");
    if (T == 0) return 0;
    if (K == 0) return fail_msg("gsr_edit_fit_sums: no anchors");
    if (!src || !dst || !workspace || !out) return fail_msg("gsr_edit_fit_sums: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    const int n_wg = reduce_workgroups(K);
    double* ws = (double*)workspace;
    edit_fit_centroid_kernel<<<dim3(n_wg, T), ED_BLOCK, 0, st>>>(K, src, dst, ws);
    GSR_CHECK_LAUNCH("edit_fit_centroid_kernel");
    edit_fit_cross_kernel<<<dim3(n_wg, T), ED_BLOCK, 0, st>>>(K, src, dst, ws);
    GSR_CHECK_LAUNCH("edit_fit_cross_kernel");
    edit_fit_finish_kernel<<<T, ED_BLOCK, 0, st>>>(n_wg, ws, out);
    GSR_CHECK_LAUNCH("edit_fit_finish_kernel");
    return 0;
}

int gsr_edit_transform_points(long long n, int stride, int offset, float* x, const double* R, const double* t, int* err,
                              gsr_stream_t stream)
{
    (void)err;
    clear_error();
    if (n < 0) return fail_msg("gsr_edit_transform_points: negative size");
    if (stride < 3 || offset < 0 || offset + 3 > stride) return fail_msg("gsr_edit_transform_points: columns outside the row");
    if (n > (long long)0x7fffffff * ED_BLOCK) return fail_msg("gsr_edit_transform_points: too many rows for one launch");
    if (!R) return fail_msg("gsr_edit_transform_points: required pointer is null");
    if (n == 0) return 0;
    if (!x) return fail_msg("gsr_edit_transform_points: required pointer is null");
    Rigid m;
    for (int i = 0; i < 9; ++i) m.r[i] = R[i];
    for (int i = 0; i < 3; ++i) m.t[i] = t ? t[i] : 0.;
    edit_transform_kernel<<<mesh_blocks(n), ED_BLOCK, 0, (hipStream_t)stream>>>(n, stride, offset, x, m, t != nullptr);
    GSR_CHECK_LAUNCH("edit_transform_kernel");
    return 0;
}

int gsr_edit_rotate_sh(int N, int M, const double* D, const float* rest_in, float* rest_out, int* err, gsr_stream_t stream)
{
    (void)err;
    clear_error();
    if (N < 0) return fail_msg("gsr_edit_rotate_sh: negative size");
    if (M != 4 && M != 9 && M != 16) return fail_msg("gsr_edit_rotate_sh: M must be 4, 9 or 16 (sh_levels 2, 3 or 4)");
    if (N == 0) return 0;
    if (!D || !rest_in || !rest_out) return fail_msg("gsr_edit_rotate_sh: required pointer is null");
    if (((size_t)rest_in | (size_t)rest_out) & 15) return fail_msg("gsr_edit_rotate_sh: rest_in and rest_out must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)((N + SH_GAUSS - 1) / SH_GAUSS);
    if (M == 4) edit_rotate_sh_kernel<2><<<grid, SH_BLOCK, 0, st>>>(N, D, rest_in, rest_out);
    else if (M == 9) edit_rotate_sh_kernel<3><<<grid, SH_BLOCK, 0, st>>>(N, D, rest_in, rest_out);
    else edit_rotate_sh_kernel<4><<<grid, SH_BLOCK, 0, st>>>(N, D, rest_in, rest_out);
    GSR_CHECK_LAUNCH("edit_rotate_sh_kernel");
    return 0;
}

int gsr_edit_faces_in_halfspaces(int F, int V, const int* faces, const float* verts, int n_groups, const int* group_sizes,
                                 const double* planes, unsigned char* mask, int* err, gsr_stream_t stream)
{
    clear_error();
    if (F < 0 || V < 0) return fail_msg("gsr_edit_faces_in_halfspaces: negative size");
    if (n_groups < 1 || n_groups > HS_MAX_GROUPS) return fail_msg("gsr_edit_faces_in_halfspaces: between 1 and 16 groups");
    if (!group_sizes || !planes) return fail_msg("gsr_edit_faces_in_halfspaces: required pointer is null");
    HalfSpaces hs;
    hs.n_groups = n_groups;
    hs.start[0] = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (group_sizes[g] < 1 || group_sizes[g] > HS_MAX_PLANES - hs.start[g])
            return fail_msg("gsr_edit_faces_in_halfspaces: a group needs a plane, and there are at most 64 planes in all");
        hs.start[g + 1] = hs.start[g] + group_sizes[g];
    }
    for (int j = 0; j < hs.start[n_groups]; ++j)
        for (int k = 0; k < 4; ++k) hs.p[j][k] = planes[4 * j + k];
    if (F == 0) return 0;
    if (!faces || !mask || !err || (V > 0 && !verts)) return fail_msg("gsr_edit_faces_in_halfspaces: required pointer is null");
    edit_halfspaces_kernel<<<mesh_blocks(F), ED_BLOCK, 0, (hipStream_t)stream>>>(F, V, faces, verts, hs, mask, err);
    GSR_CHECK_LAUNCH("edit_halfspaces_kernel");
    return 0;
}

int gsr_edit_gather_rows(int n_faces, int F, const int* kept, int G, int n_tables, const void* const* src, void* const* dst,
                         const int* row_words, int* err, gsr_stream_t stream)
{
    clear_error();
    if (n_faces < 0 || F < 0) return fail_msg("gsr_edit_gather_rows: negative size");
    if (G < 1) return fail_msg("gsr_edit_gather_rows: G must be positive");
    if (n_tables < 1 || n_tables > GR_MAX) return fail_msg("gsr_edit_gather_rows: between 1 and 8 tables");
    if (!src || !dst || !row_words) return fail_msg("gsr_edit_gather_rows: required pointer is null");
    GatherTable tb;
    tb.n = n_tables;
    tb.first[0] = 0;
    for (int e = 0; e < n_tables; ++e) {
        if (row_words[e] < 1 || (long long)row_words[e] * G > 0x7fffffff) return fail_msg("gsr_edit_gather_rows: a row width is not positive");
        tb.words[e] = row_words[e] * G;
        const long long blocks = ((long long)n_faces * tb.words[e] + ED_BLOCK - 1) / ED_BLOCK;
        if (tb.first[e] + blocks > 0x7fffffffLL) return fail_msg("gsr_edit_gather_rows: too many rows for one launch");
        tb.first[e + 1] = tb.first[e] + (unsigned)blocks;
        tb.src[e] = (const unsigned*)src[e];
        tb.dst[e] = (unsigned*)dst[e];
        if (n_faces > 0 && (!src[e] || !dst[e])) return fail_msg("gsr_edit_gather_rows: required pointer is null");
    }
    for (int e = n_tables; e < GR_MAX; ++e) { tb.src[e] = nullptr; tb.dst[e] = nullptr; tb.words[e] = 0; tb.first[e + 1] = tb.first[n_tables]; }
    if (n_faces == 0) return 0;
    if (!kept || !err) return fail_msg("gsr_edit_gather_rows: required pointer is null");
    edit_gather_kernel<<<tb.first[n_tables], ED_BLOCK, 0, (hipStream_t)stream>>>(n_faces, F, kept, tb, err);
    GSR_CHECK_LAUNCH("edit_gather_kernel");
    return 0;
}

int gsr_edit_paint(int N, int G, int F, int V, const int* faces, const float* verts, const float* bary, int n_tri, const double* tri,
                   int h, int w, int C, const unsigned char* texture, int mode, double bary_slack, double max_dist, int shrink,
                   float shrink_scale, int alpha_min, float* scales, float* sh_dc, int* stats, int* err, gsr_stream_t stream)
{
    clear_error();
    if (N < 0 || F < 0 || V < 0) return fail_msg("gsr_edit_paint: negative size");
    if (G < 1) return fail_msg("gsr_edit_paint: G must be positive");
    if (n_tri < 1 || n_tri > PT_MAX_TRI) return fail_msg("gsr_edit_paint: between 1 and 64 triangles");
    if (h < 1 || w < 1 || (long long)h * w * 4 > 0x7fffffff) return fail_msg("gsr_edit_paint: the texture's size must be positive");
    if (C != 1 && C != 3 && C != 4) return fail_msg("gsr_edit_paint: the texture has 1, 3 or 4 channels");
    if (mode != 0 && mode != 1) return fail_msg("gsr_edit_paint: mode is 0 (multiply) or 1 (replace)");
    if (mode == 1 && C == 1) return fail_msg("gsr_edit_paint: replace needs a texture of 3 or 4 channels");
    if (!stats) return fail_msg("gsr_edit_paint: required pointer is null");
    if (N > 0 && (!faces || !verts || !bary || !tri || !texture || !scales || !sh_dc || !err))
        return fail_msg("gsr_edit_paint: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    GSR_CHECK(hipMemsetAsync(stats, 0, (2 + n_tri) * sizeof(int), st));
    if (N == 0) return 0;
    PaintArgs a = {N, G, F, V, n_tri, h, w, C, mode, shrink != 0, alpha_min, shrink_scale, bary_slack, max_dist};
    edit_paint_kernel<<<mesh_blocks(N), ED_BLOCK, 0, st>>>(a, faces, verts, bary, tri, texture, scales, sh_dc, stats, err);
    GSR_CHECK_LAUNCH("edit_paint_kernel");
    return 0;
}

}  // extern "C"
