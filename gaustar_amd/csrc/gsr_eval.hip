// gsr_eval.hip -- scoring a result: the exact distance from points to a triangle mesh, area-weighted surface samples, the
// statistics of a set of distances and an image pair's sum of squared differences: gaustar_amd.evaluate (mesh distance, Chamfer,
// F-score, PSNR).  The reference scores from PNG directories with torchvision and lpips (gaussian_splatting/metrics.py,
// utils/image_utils.py) and has no geometric score; nothing here mirrors a library, the definitions are include/gsr.h's own.
//   face records        eval_gather_kernel         tri [9,F] f64: a, b, c of every face, coordinate-major, NaN for a face left out
//   closest point       eval_closest_kernel        the one O(K F) step: gsr_surface.h's tnn_search -- 256 threads, 16 queries per
//                                                  workgroup, the records staged through LDS in tiles of 512 faces (9 x 512
//                                                  doubles = 36 KiB) and split 16 ways among the lanes -- with the region test
//                                                  written as selects, so lanes that hold different faces do not diverge, one
//                                                  reciprocal per pair, and the (d2, face) minimum; the winner's barycentrics,
//                                                  point and the one square root are formed once per query at the end
//   areas, samples      eval_areas_kernel, eval_sample_kernel     which face a sample takes is decided in integers
//   distance statistics eval_stats_kernel          sums by gsr_reduce.h, the maximum and the counts by integer atomics
//   image SSE           eval_image_sse_kernel      f32 difference and square, f64 sum by gsr_reduce.h, an integer count
// All geometry is float64 without contraction, every operation in the order include/gsr.h states.  No float atomics, no scratch.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_reduce.h"
#include "gsr_surface.h"

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int EV_BLOCK = MESH_BLOCK;
constexpr int EV_TILE = 512;        // faces staged in LDS at once: 9 x 512 doubles = 36 KiB
constexpr int EV_MAX_THR = 8;       // thresholds of one gsr_eval_distance_stats call

// The closest point of triangle (a, b, c) to p, as include/gsr.h states it -> the squared distance; v, w its barycentrics on
// b and c (u is formed by the caller), q the point.  Every region's (nv, nw, den) is chosen by selects.
__device__ __forceinline__ double closest_on_face(D3 p, D3 a, D3 b, D3 c, double& v, double& w, D3& q)
{
    const D3 ab = sub3(b, a), ac = sub3(c, a), ap = sub3(p, a), bp = sub3(p, b), cp = sub3(p, c);
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4, e = d4 - d3, g = d5 - d6;
    const bool rA = (d1 <= 0.) & (d2 <= 0.);
    const bool rB = (d3 >= 0.) & (d4 <= d3);
    const bool rAB = (vc <= 0.) & (d1 >= 0.) & (d3 <= 0.);
    const bool rC = (d6 >= 0.) & (d5 <= d6);
    const bool rAC = (vb <= 0.) & (d2 >= 0.) & (d6 <= 0.);
    const bool rBC = (va <= 0.) & (e >= 0.) & (g >= 0.);
    double nv = vb, nw = vc, den = (va + vb) + vc;           // inside
    nw = rBC ? e : nw;   den = rBC ? e + g : den;            // (nv is not read on BC)
    nv = rAC ? 0. : nv;  nw = rAC ? d2 : nw;  den = rAC ? d2 - d6 : den;
    nv = rC ? 0. : nv;   nw = rC ? 1. : nw;   den = rC ? 1. : den;
    nv = rAB ? d1 : nv;  nw = rAB ? 0. : nw;  den = rAB ? d1 - d3 : den;
    nv = rB ? 1. : nv;   nw = rB ? 0. : nw;   den = rB ? 1. : den;
    nv = rA ? 0. : nv;   nw = rA ? 0. : nw;   den = rA ? 1. : den;
    const bool bc = rBC & !(rA | rB | rAB | rC | rAC);
    const double r = 1.0 / den;
    w = nw * r;
    const double v_bc = 1.0 - w, v_else = nv * r;            // (both formed, then a select: a ternary of expressions becomes a branch)
    v = bc ? v_bc : v_else;
    q = {a.x + (ab.x * v + ac.x * w), a.y + (ab.y * v + ac.y * w), a.z + (ab.z * v + ac.z * w)};
    const D3 d = sub3(p, q);
    return dot3(d, d);
}

// tri [9,F]: row 3 i + k = coordinate k of vertex i of every face; NaN (and err) for a face left out
__global__ void __launch_bounds__(EV_BLOCK) eval_gather_kernel(int F, int V, const int* __restrict__ faces, const double* __restrict__ verts,
                                                               double* __restrict__ tri, int* __restrict__ err)
{
    const int f = blockIdx.x * EV_BLOCK + threadIdx.x;
    if (f >= F) return;
    const double nan = __builtin_nan("");
    D3 t0 = {nan, nan, nan}, t1 = t0, t2 = t0, a, b, c;
    if (face_verts(faces, verts, f, V, a, b, c, err)) { t0 = a; t1 = b; t2 = c; }
    const size_t n = (size_t)F;
    tri[f] = t0.x; tri[n + f] = t0.y; tri[2 * n + f] = t0.z;
    tri[3 * n + f] = t1.x; tri[4 * n + f] = t1.y; tri[5 * n + f] = t1.z;
    tri[6 * n + f] = t2.x; tri[7 * n + f] = t2.y; tri[8 * n + f] = t2.z;
}

// slot s < n = min(S, *n_live) (S where n_live == NULL) is query k = list ? list[s] : s, k in [0, K).  Per slot: face = the
// lowest j among those with the smallest d2, bary (u, v, w), closest q, dist = sqrt(d2).  grid = ceil(S / 16): the surplus
// workgroups exit on n.  A pair whose d2 is NaN ranks nothing; a slot for which no face ranks gets face -1, dist +inf, NaN
// bary and closest, and err bit 1.
__global__ void __launch_bounds__(TNN_BLOCK) eval_closest_kernel(int S, const int* __restrict__ list, const int* __restrict__ n_live, int K,
                                                                 int F, const double* __restrict__ pts, const double* __restrict__ tri,
                                                                 int* __restrict__ face, double* __restrict__ bary,
                                                                 double* __restrict__ closest, double* __restrict__ dist,
                                                                 int* __restrict__ err)
{
    int n = n_live ? *n_live : S;
    n = n < S ? n : S;
    if (blockIdx.x * TNN_QUERIES >= n) return;               // (the whole workgroup, ahead of tnn_search's barriers)
    const int slot = blockIdx.x * TNN_QUERIES + tnn_query();
    const bool live = slot < n;
    const double nan = __builtin_nan("");
    D3 p = {nan, nan, nan};                                  // (a slot without a query ranks nothing)
    if (live) {
        const int k = list ? list[slot] : slot;
        if ((unsigned)k < (unsigned)K) p = load3(pts, (size_t)k);
        else if (tnn_owner()) atomicOr(err, MESH_ERR_INDEX);
    }
    double bd;
    int bi;
    tnn_search<9, EV_TILE, 1>(
        F, bd, bi,
        [&](double (*tile)[EV_TILE], int base, int m) {
            for (int e = threadIdx.x; e < 9 * m; e += TNN_BLOCK) {
                const int row = e / m, j = e - row * m;
                tile[row][j] = tri[(size_t)row * F + base + j];
            }
        },
        [&](const double (*tile)[EV_TILE], int j) {
            const D3 a = {tile[0][j], tile[1][j], tile[2][j]}, b = {tile[3][j], tile[4][j], tile[5][j]},
                     c = {tile[6][j], tile[7][j], tile[8][j]};
            double v, w;
            D3 q;
            return closest_on_face(p, a, b, c, v, w, q);
        });
    if (!(tnn_owner() && live)) return;
    D3 uvw = {nan, nan, nan}, q = {nan, nan, nan};
    double d = __builtin_inf();
    if (bi == TNN_NONE) {
        atomicOr(err, MESH_ERR_NAN);
        bi = -1;
    } else {
        const size_t Fs = (size_t)F, f = (size_t)bi;
        const D3 a = {tri[f], tri[Fs + f], tri[2 * Fs + f]}, b = {tri[3 * Fs + f], tri[4 * Fs + f], tri[5 * Fs + f]},
                 c = {tri[6 * Fs + f], tri[7 * Fs + f], tri[8 * Fs + f]};
        double v, w;
        const double d2 = closest_on_face(p, a, b, c, v, w, q);
        double u = (1.0 - v) - w;
        u = u < 0. ? 0. : u;
        uvw = {u, v, w};
        d = sqrt(d2);
    }
    face[slot] = bi;
    store3(bary, (size_t)slot, uvw);
    store3(closest, (size_t)slot, q);
    dist[slot] = d;
}

// regions.face_areas' statement on f64 vertices: u = v1 - v0, w = v2 - v1, c = u x w, area = 0.5 sqrt((cx cx + cy cy) + cz cz);
// 0 for a face left out
__global__ void __launch_bounds__(EV_BLOCK) eval_areas_kernel(int F, int V, const int* __restrict__ faces, const double* __restrict__ verts,
                                                              double* __restrict__ area, int* __restrict__ err)
{
    const int f = blockIdx.x * EV_BLOCK + threadIdx.x;
    if (f >= F) return;
    D3 t0, t1, t2;
    double out = 0.0;
    if (face_verts(faces, verts, f, V, t0, t1, t2, err)) {
        const D3 u = sub3(t1, t0), w = sub3(t2, t1);
        const double cx = u.y * w.z - u.z * w.y, cy = u.z * w.x - u.x * w.z, cz = u.x * w.y - u.y * w.x;
        out = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
    }
    area[f] = out;
}

// splitmix64's finaliser
__device__ __forceinline__ unsigned long long mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// cum [F] int64 = the inclusive scan of the integer weights.  Sample k: the stratum's point t_k, the lowest face whose cum is
// above it, the barycentrics from the hash of (seed, k), the point by bary_to_point.
__global__ void __launch_bounds__(EV_BLOCK) eval_sample_kernel(int n, int F, int V, const int* __restrict__ faces,
                                                               const double* __restrict__ verts, const long long* __restrict__ cum,
                                                               unsigned long long seed, int* __restrict__ face_ids,
                                                               double* __restrict__ bary, double* __restrict__ points, int* __restrict__ err)
{
    const int k = blockIdx.x * EV_BLOCK + threadIdx.x;
    if (k >= n) return;
    const double nan = __builtin_nan("");
    D3 b = {nan, nan, nan}, pt = {nan, nan, nan}, t0, t1, t2;
    int f = 0;
    const long long W = cum[F - 1];
    if (W < (long long)n) atomicOr(err, MESH_ERR_DEGENERATE);   // (the weights are not this file's: max w >= 2^31 > n)
    else {
        const long long q = W / n, r = W % n;
        const long long tk = (long long)k * q + ((long long)k < r ? (long long)k : r) + q / 2;
        int lo = 0, hi = F - 1;
        while (lo < hi) {
            const int mid = (int)(((long long)lo + hi) >> 1);
            if (cum[mid] > tk) hi = mid; else lo = mid + 1;
        }
        f = lo;
        const unsigned long long z = mix64(seed + (unsigned long long)(k + 1ll) * 0x9E3779B97F4A7C15ull);
        double s = ((double)(z >> 32) + 0.5) * 0x1p-32, t = ((double)(z & 0xffffffffull) + 0.5) * 0x1p-32;
        if (s + t > 1.0) { s = 1.0 - s; t = 1.0 - t; }
        if (face_verts(faces, verts, f, V, t0, t1, t2, err)) {
            b = {(1.0 - s) - t, s, t};
            pt = bary_to_point(t0, t1, t2, b);
        }
    }
    face_ids[k] = f;
    store3(bary, (size_t)k, b);
    store3(points, (size_t)k, pt);
}

__device__ __forceinline__ long long wave_sum_ll(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// out (cleared before): word 2 = the largest d as its bit pattern, word 3 + t = how many d < thr[t]; the sums of d and of d d
// go through gsr_reduce.h.  A thread takes d[i], i = its global index, + the grid's size, ... in that order.
__global__ void __launch_bounds__(RED_BLOCK) eval_stats_kernel(long long K, const double* __restrict__ d, int T, const double* __restrict__ thr,
                                                               double* __restrict__ partials, unsigned long long* __restrict__ out)
{
    double s[2] = {0.0, 0.0}, tau[EV_MAX_THR];
    long long cnt[EV_MAX_THR];
    unsigned long long mx = 0;
#pragma unroll
    for (int t = 0; t < EV_MAX_THR; ++t) { tau[t] = t < T ? thr[t] : -__builtin_inf(); cnt[t] = 0; }
    const long long stride = (long long)gridDim.x * RED_BLOCK;
    for (long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x; i < K; i += stride) {
        const double x = d[i];
        s[0] += x;
        s[1] += x * x;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
        mx = bits > mx ? bits : mx;
#pragma unroll
        for (int t = 0; t < EV_MAX_THR; ++t) cnt[t] += x < tau[t] ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = (unsigned long long)__shfl_down((long long)mx, o, 64);
        mx = other > mx ? other : mx;
    }
#pragma unroll
    for (int t = 0; t < EV_MAX_THR; ++t) cnt[t] = wave_sum_ll(cnt[t]);
    if ((threadIdx.x & 63) == 0) {
        if (mx) atomicMax(out + 2, mx);
#pragma unroll
        for (int t = 0; t < EV_MAX_THR; ++t)
            if (t < T && cnt[t]) atomicAdd(out + 3 + t, (unsigned long long)cnt[t]);
    }
    block_partials<2>(s, partials);
}

// pred, gt [C,H,W] f32 with element strides; mask [H,W] bytes, contiguous, or NULL.  Per element of a pixel the mask keeps:
// p = clamp01 ? (pred < 0 ? 0 : pred > 1 ? 1 : pred) : pred; e = p - gt and e e in f32; the square widened and summed.
// count (cleared before) = the elements taken.
__global__ void __launch_bounds__(RED_BLOCK) eval_image_sse_kernel(int C, int H, int W, const float* __restrict__ pred, long long ps0,
                                                                   long long ps1, long long ps2, const float* __restrict__ gt, long long gs0,
                                                                   long long gs1, long long gs2, const unsigned char* __restrict__ mask,
                                                                   int clamp01, double* __restrict__ partials,
                                                                   unsigned long long* __restrict__ count)
{
    double s[1] = {0.0};
    long long taken = 0;
    const long long hw = (long long)H * W, total = hw * C, stride = (long long)gridDim.x * RED_BLOCK;
    for (long long i = (long long)blockIdx.x * RED_BLOCK + threadIdx.x; i < total; i += stride) {
        const long long c = i / hw, px = i - c * hw, y = px / W, x = px - y * W;
        if (mask && !mask[px]) continue;
        float p = pred[c * ps0 + y * ps1 + x * ps2];
        if (clamp01) p = p < 0.f ? 0.f : (p > 1.f ? 1.f : p);
        const float e = p - gt[c * gs0 + y * gs1 + x * gs2];
        const float sq = e * e;
        s[0] += (double)sq;
        ++taken;
    }
    taken = wave_sum_ll(taken);
    if ((threadIdx.x & 63) == 0 && taken) atomicAdd(count, (unsigned long long)taken);
    block_partials<1>(s, partials);
}

template <int N>
__global__ void __launch_bounds__(RED_BLOCK) eval_total_kernel(int n_wg, const double* __restrict__ partials, double* __restrict__ out)
{
    double t[N];
    tree_total<N>(n_wg, partials, t);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = t[k];
    }
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

int gsr_eval_tile(void) { return EV_TILE; }
int gsr_eval_queries(void) { return TNN_QUERIES; }
int gsr_eval_max_thresholds(void) { return EV_MAX_THR; }
size_t gsr_eval_workspace_bytes(void) { return reduce_workspace_bytes(); }

int gsr_eval_gather(int F, int V, const int* faces, const double* verts, double* tri, int* err, gsr_stream_t stream)
{
    clear_error();
    if (F < 0 || V < 0) return fail_msg("gsr_eval_gather: negative size");
    if (F == 0) return 0;
    if (!faces || !tri || !err || (V > 0 && !verts)) return fail_msg("gsr_eval_gather: required pointer is null");
    eval_gather_kernel<<<mesh_blocks(F), EV_BLOCK, 0, (hipStream_t)stream>>>(F, V, faces, verts, tri, err);
    GSR_CHECK_LAUNCH("eval_gather_kernel");
    return 0;
}

int gsr_eval_closest(int S, const int* list, const int* n_live, int K, int F, const double* queries, const double* tri, int* face,
                     double* bary, double* closest, double* dist, int* err, gsr_stream_t stream)
{
    clear_error();
    if (S < 0 || K < 0 || F < 0) return fail_msg("gsr_eval_closest: negative size");
    if (S == 0) return 0;
    if (F == 0) return fail_msg("gsr_eval_closest: no faces");
    if (!tri || !face || !bary || !closest || !dist || !err || (K > 0 && !queries))
        return fail_msg("gsr_eval_closest: required pointer is null");
    eval_closest_kernel<<<(unsigned)((S + TNN_QUERIES - 1) / TNN_QUERIES), TNN_BLOCK, 0, (hipStream_t)stream>>>(
        S, list, n_live, K, F, queries, tri, face, bary, closest, dist, err);
    GSR_CHECK_LAUNCH("eval_closest_kernel");
    return 0;
}

int gsr_eval_areas(int F, int V, const int* faces, const double* verts, double* area, int* err, gsr_stream_t stream)
{
    clear_error();
    if (F < 0 || V < 0) return fail_msg("gsr_eval_areas: negative size");
    if (F == 0) return 0;
    if (!faces || !area || !err || (V > 0 && !verts)) return fail_msg("gsr_eval_areas: required pointer is null");
    eval_areas_kernel<<<mesh_blocks(F), EV_BLOCK, 0, (hipStream_t)stream>>>(F, V, faces, verts, area, err);
    GSR_CHECK_LAUNCH("eval_areas_kernel");
    return 0;
}

int gsr_eval_sample(int n, int F, int V, const int* faces, const double* verts, const long long* cum, unsigned long long seed,
                    int* face_ids, double* bary, double* points, int* err, gsr_stream_t stream)
{
    clear_error();
    if (n < 0 || F < 0 || V < 0) return fail_msg("gsr_eval_sample: negative size");
    if (n == 0) return 0;
    if (F == 0) return fail_msg("gsr_eval_sample: no faces");
    if (!faces || !cum || !face_ids || !bary || !points || !err || (V > 0 && !verts))
        return fail_msg("gsr_eval_sample: required pointer is null");
    eval_sample_kernel<<<mesh_blocks(n), EV_BLOCK, 0, (hipStream_t)stream>>>(n, F, V, faces, verts, cum, seed, face_ids, bary, points, err);
    GSR_CHECK_LAUNCH("eval_sample_kernel");
    return 0;
}

int gsr_eval_distance_stats(long long K, const double* dist, int T, const double* thresholds, void* workspace, void* out,
                            gsr_stream_t stream)
{
    clear_error();
    if (K < 0 || T < 0 || T > EV_MAX_THR) return fail_msg("gsr_eval_distance_stats: K < 0, or T outside [0, 8]");
    if (!workspace || !out || (K > 0 && !dist) || (T > 0 && !thresholds))
        return fail_msg("gsr_eval_distance_stats: required pointer is null");
    if (!aligned8(workspace) || !aligned8(out) || !aligned8(dist) || !aligned8(thresholds))
        return fail_msg("gsr_eval_distance_stats: arrays must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    GSR_CHECK(hipMemsetAsync(out, 0, (3 + (size_t)T) * 8, st));
    const int n_wg = K > 0 ? reduce_workgroups(K) : 1;      // (K = 0: one workgroup writes the zero partials)
    double* partials = static_cast<double*>(workspace);
    eval_stats_kernel<<<(unsigned)n_wg, RED_BLOCK, 0, st>>>(K, dist, T, thresholds, partials, static_cast<unsigned long long*>(out));
    eval_total_kernel<2><<<1, RED_BLOCK, 0, st>>>(n_wg, partials, static_cast<double*>(out));
    GSR_CHECK_LAUNCH("eval stats kernels");
    return 0;
}

int gsr_eval_image_sse(int C, int H, int W, const float* pred, long long ps0, long long ps1, long long ps2, const float* gt,
                       long long gs0, long long gs1, long long gs2, const unsigned char* mask, int clamp01, void* workspace, void* out,
                       gsr_stream_t stream)
{
    clear_error();
    if (C <= 0 || H <= 0 || W <= 0) return fail_msg("gsr_eval_image_sse: sizes must be positive");
    if (!pred || !gt || !workspace || !out) return fail_msg("gsr_eval_image_sse: required pointer is null");
    if (!aligned8(workspace) || !aligned8(out)) return fail_msg("gsr_eval_image_sse: workspace and out must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    GSR_CHECK(hipMemsetAsync(out, 0, 16, st));
    const int n_wg = reduce_workgroups((long long)C * H * W);
    double* partials = static_cast<double*>(workspace);
    eval_image_sse_kernel<<<(unsigned)n_wg, RED_BLOCK, 0, st>>>(C, H, W, pred, ps0, ps1, ps2, gt, gs0, gs1, gs2, mask, clamp01, partials,
                                                                 static_cast<unsigned long long*>(out) + 1);
    eval_total_kernel<1><<<1, RED_BLOCK, 0, st>>>(n_wg, partials, static_cast<double*>(out));
    GSR_CHECK_LAUNCH("eval image kernels");
    return 0;
}

}  // extern "C"
