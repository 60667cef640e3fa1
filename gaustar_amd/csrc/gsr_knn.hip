// gsr_knn.hip -- exact K-nearest-neighbour search, 1 <= K <= 32, of f32 points (pytorch3d's knn_points as sugar_model.py:49, :253,
// :862, :877, :1014 and warp_mesh.py:199-213 call it; simple-knn's distCUDA2, simple_knn.cu:147-183) and what the callers do with
// the rows: the mean of three squared distances, a voxel's mean, the distance-weighted mean of interpolate_in_voxel.
//
// The rules are the ones tests/topo_ref.py::knn and gsr_topo.hip state for pytorch3d, restated in tests/knn_ref.py: with
// d = query - candidate in f32, d2 = (dx dx + dy dy) + dz dz without contraction; a row holds the K smallest pairs in
// ascending (d2, candidate index) order; slots beyond the eligible candidates hold (-1, +inf); a point with a non-finite
// coordinate is never a neighbour and has, as a query, an empty row.  The result is the exhaustive search's bit for bit,
// whatever the order the work is done in:
//   prepare  knn_prepare_kernel: the candidates in the caller's sorted order (a space-filling curve: gaustar_amd/knn.py) as
//            float4 (xyz, index bits), a non-finite one as NaN, and the box of every tile of KN_TILE consecutive ones;
//   search   knn_search_kernel<L>: one-wave workgroups of KN_QUERIES consecutive sorted queries, one per lane.  Seed: the K
//            best of the 2 KN_SEED + 1 sorted candidates around the query's sorted position; their K-th distance tau bounds
//            the true K-th from above.  Then every tile in order: a tile is skipped iff its box is farther than the lane's
//            current bound for EVERY lane (a wave-uniform branch); the lower bound repeats d2's operations in d2's order with
//            0 for an axis inside the box, so by the monotonicity of rounding it never exceeds the d2 of a point in the box.  A
//            tile that stays goes through LDS (every lane reads the same address: a broadcast) and a candidate is offered
//            only when d2 <= bound = min(tau, the list's K-th), the rare divergent branch.
// The lists are register arrays of L = 4 / 8 / 16 / 32 entries indexed by unrolled loops only (a runtime index would put
// them in scratch); K is rounded up to an instance whose first L - K slots are held by sentinels, and the last K are written.
// No float atomics; the two counters of `stats` are integer atomics, one each per workgroup.
#include "../../include/gsr.h"
#include "gsr_entry.h"

#include <cfloat>
#include <cstdint>

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int KN_TILE = 64;       // candidates per tile (one float4 per lane of the loading wave)
constexpr int KN_SEED = 16;       // sorted candidates on either side of a query's position in the seed (33 >= 32 + self)
constexpr int KN_QUERIES = 64;    // queries per workgroup = one wave
constexpr int KN_MAX_K = 32;
constexpr int KN_BLOCK = 256;     // the per-row kernels
constexpr int KN_EMPTY = 0x7fffffff;

// A list of K entries in an array of L: the first L - K slots hold (-inf, -1), below every offer, so the K live entries are
// the LAST K slots and the K-th best is always bd[L - 1], a register known at compile time.
template <int L>
__device__ __forceinline__ void kn_init(float (&bd)[L], int (&bi)[L], int K)
{
#pragma unroll
    for (int k = 0; k < L; ++k) { bd[k] = k < L - K ? -INFINITY : INFINITY; bi[k] = k < L - K ? -1 : KN_EMPTY; }
}

// (d, id) into the list ordered by (distance, index); a NaN distance never enters
template <int L>
__device__ __forceinline__ void kn_insert(float d, int id, float (&bd)[L], int (&bi)[L])
{
    if (d < bd[L - 1] || (d == bd[L - 1] && id < bi[L - 1])) {
#pragma unroll
        for (int k = 0; k < L; ++k) {
            if (d < bd[k] || (d == bd[k] && id < bi[k])) {
                const float td = bd[k]; const int ti = bi[k];
                bd[k] = d; bi[k] = id; d = td; id = ti;
            }
        }
    }
}

__device__ __forceinline__ float kn_dist(float qx, float qy, float qz, float cx, float cy, float cz)
{
    const float dx = qx - cx, dy = qy - cy, dz = qz - cz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ float kn_axis(float q, float lo, float hi) { return q < lo ? q - lo : (q > hi ? q - hi : 0.f); }

__device__ __forceinline__ bool kn_finite(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__global__ void __launch_bounds__(KN_TILE) knn_prepare_kernel(int M, const float* __restrict__ cand, const long long* __restrict__ order,
                                                              float4* __restrict__ out, float4* __restrict__ boxes)
{
    const int pos = blockIdx.x * KN_TILE + threadIdx.x;   // (the copy is padded to whole tiles)
    float x = NAN, y = NAN, z = NAN;
    int id = KN_EMPTY;
    bool ok = false;
    if (pos < M) {
        const long long o = order[pos];
        if (o >= 0 && o < M) {
            id = (int)o;
            x = cand[3 * o]; y = cand[3 * o + 1]; z = cand[3 * o + 2];
            ok = kn_finite(x, y, z);
            if (!ok) x = y = z = NAN;
        }
    }
    out[pos] = make_float4(x, y, z, __int_as_float(id));
    float lo[3] = {ok ? x : INFINITY, ok ? y : INFINITY, ok ? z : INFINITY};
    float hi[3] = {ok ? x : -INFINITY, ok ? y : -INFINITY, ok ? z : -INFINITY};
#pragma unroll
    for (int m = KN_TILE / 2; m > 0; m >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], m, KN_TILE));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], m, KN_TILE));
        }
    }
    if (threadIdx.x == 0) {   // (a tile without a finite point: lo = +inf, hi = -inf, infinitely far from every query)
        boxes[2 * blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.f);
        boxes[2 * blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
    }
}

template <int L>
__global__ void __launch_bounds__(KN_QUERIES) knn_search_kernel(int N, int M, int K, const float* __restrict__ queries,
                                                                const long long* __restrict__ qorder, const long long* __restrict__ qpos,
                                                                const float4* __restrict__ cand, const float4* __restrict__ boxes,
                                                                int exclude_self, int cull, int* __restrict__ idx, float* __restrict__ d2,
                                                                unsigned long long* __restrict__ stats)
{
    __shared__ float4 tile[KN_TILE];
    const int lane = threadIdx.x;
    const int s = blockIdx.x * KN_QUERIES + lane;
    const int nlive = min(KN_QUERIES, N - (int)blockIdx.x * KN_QUERIES);
    long long qi = s < N ? qorder[s] : -1;
    const bool live = qi >= 0 && qi < N;
    if (!live) qi = 0;
    const float qx = live ? queries[3 * qi] : NAN, qy = live ? queries[3 * qi + 1] : NAN, qz = live ? queries[3 * qi + 2] : NAN;
    const bool qok = live && kn_finite(qx, qy, qz);
    const int self = exclude_self ? (int)qi : -1;

    float bd[L];
    int bi[L];
    kn_init(bd, bi, K);
    float tau = INFINITY;
    unsigned int seed_pairs = 0;
    if (cull && qok) {
        const long long p = qpos[s];
        const int lo = (int)max(0ll, min((long long)M, p - KN_SEED)), hi = (int)max(0ll, min((long long)M, p + KN_SEED + 1));
        for (int j = lo; j < hi; ++j) {
            const float4 c = cand[j];
            const int id = __float_as_int(c.w);
            if (id != self) kn_insert(kn_dist(qx, qy, qz, c.x, c.y, c.z), id, bd, bi);
        }
        seed_pairs = (unsigned int)(hi - lo);
        tau = bd[L - 1];   // (inf with fewer than K eligible candidates in the window: no bound)
        kn_init(bd, bi, K);
    }
    float bound = qok ? tau : -1.f;   // (a query that is not finite is offered nothing)

    const int ntiles = (M + KN_TILE - 1) / KN_TILE;
    unsigned long long pairs = 0;
    unsigned int skipped = 0;
    for (int t = 0; t < ntiles; ++t) {
        if (cull) {
            const float4 blo = boxes[2 * t], bhi = boxes[2 * t + 1];
            const float ax = kn_axis(qx, blo.x, bhi.x), ay = kn_axis(qy, blo.y, bhi.y), az = kn_axis(qz, blo.z, bhi.z);
            const float lb = (ax * ax + ay * ay) + az * az;
            if (!__any(qok && !(lb > bound))) { ++skipped; continue; }
        }
        __syncthreads();
        tile[lane] = cand[(size_t)t * KN_TILE + lane];
        __syncthreads();
        const int n = min(KN_TILE, M - t * KN_TILE);
        pairs += (unsigned long long)n * nlive;
        for (int j = 0; j < n; ++j) {
            const float4 c = tile[j];
            const float d = kn_dist(qx, qy, qz, c.x, c.y, c.z);
            if (d <= bound) {
                const int id = __float_as_int(c.w);
                if (id != self) {
                    kn_insert(d, id, bd, bi);
                    bound = fminf(tau, bd[L - 1]);
                }
            }
        }
    }
    if (live) {
        const size_t o = (size_t)qi * K;
#pragma unroll
        for (int k = 0; k < L; ++k) {
            if (k >= L - K) {
                const bool empty = bi[k] == KN_EMPTY;
                idx[o + (k - (L - K))] = empty ? -1 : bi[k];
                d2[o + (k - (L - K))] = empty ? INFINITY : bd[k];
            }
        }
    }
    if (stats) {
#pragma unroll
        for (int m = KN_QUERIES / 2; m > 0; m >>= 1) seed_pairs += __shfl_xor(seed_pairs, m, KN_QUERIES);
        if (lane == 0) {
            atomicAdd(&stats[0], pairs + seed_pairs);
            atomicAdd(&stats[1], (unsigned long long)skipped);
        }
    }
}

// simple_knn.cu:182: the mean of the three best, an empty slot at FLT_MAX as the reference's `best` starts
__global__ void __launch_bounds__(KN_BLOCK) knn_mean_d2_kernel(int N, int K, const float* __restrict__ d2, float* __restrict__ out)
{
    const int i = blockIdx.x * KN_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float* r = d2 + (size_t)i * K;
    const float a = r[0] == INFINITY ? FLT_MAX : r[0], b = r[1] == INFINITY ? FLT_MAX : r[1], c = r[2] == INFINITY ? FLT_MAX : r[2];
    out[i] = ((a + b) + c) / 3.0f;
}

// the head of every run of equal ids sums its run in sorted order
__global__ void __launch_bounds__(KN_BLOCK) knn_segment_mean_kernel(int n, int S, int C, const long long* __restrict__ ids,
                                                                    const long long* __restrict__ order, const double* __restrict__ values,
                                                                    double* __restrict__ out, int* __restrict__ count)
{
    const int i = blockIdx.x * KN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long id = ids[i];
    if (id < 0 || id >= S || (i > 0 && ids[i - 1] == id)) return;
    int m = 0;
    for (int j = i; j < n && ids[j] == id; ++j) ++m;
    for (int c = 0; c < C; ++c) {
        double sum = 0.0;
        for (int j = i; j < i + m; ++j) {
            const long long o = order[j];
            if (o >= 0 && o < n) sum += values[(size_t)o * C + c];
        }
        out[(size_t)id * C + c] = sum / m;
    }
    count[id] = m;
}

// exp(x) for x <= 0 from IEEE operations only, in a fixed order, so that tests/knn_ref.py::exp_neg repeats it bit for bit:
// x = n ln 2 + r with |r| <= 0.35, the Taylor polynomial of degree 13 by Horner's rule (its remainder is below 2^-58), times
// 2^n.  Below -700 the result is 0.
__device__ __forceinline__ double kn_exp_neg(double x)
{
    if (!(x >= -700.0)) return x != x ? x : 0.0;
    const double n = rint(x * 1.4426950408889634);
    const double r = (x - n * 0.693147180369123816490) - n * 1.90821492927058770002e-10;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 0.5;
    p = p * r + 1.0;
    p = p * r + 1.0;
    return p * __longlong_as_double(((long long)n + 1023) << 52);
}

// interpolate_in_voxel's average (warp_mesh.py:204-211); an empty slot is (index 0, distance 0), as pytorch3d pads
__global__ void __launch_bounds__(KN_BLOCK) knn_weighted_mean_kernel(int N, int K, int C, int M, const int* __restrict__ idx,
                                                                     const float* __restrict__ d2, const double* __restrict__ values,
                                                                     double inv_scale, double* __restrict__ out)
{
    const int i = blockIdx.x * KN_BLOCK + threadIdx.x;
    if (i >= N) return;
    for (int c = 0; c < C; ++c) {
        double sw = 0.0, swv = 0.0;
        for (int k = 0; k < K; ++k) {
            const int j = idx[(size_t)i * K + k];
            const bool have = j >= 0 && j < M;
            const double w = kn_exp_neg(-(double)(have ? d2[(size_t)i * K + k] : 0.f) * inv_scale) + 1e-8;
            swv += values[(size_t)(have ? j : 0) * C + c] * w;
            sw += w;
        }
        out[(size_t)i * C + c] = swv / sw;
    }
}

inline int blocks(long long n, int b) { return (int)((n + b - 1) / b); }

inline size_t tiles_of(int M) { return ((size_t)M + KN_TILE - 1) / KN_TILE; }

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

int gsr_knn_tile(void) { return KN_TILE; }
int gsr_knn_seed(void) { return KN_SEED; }
int gsr_knn_queries(void) { return KN_QUERIES; }
int gsr_knn_max_k(void) { return KN_MAX_K; }

size_t gsr_knn_workspace_bytes(int N, int M, int K)
{
    (void)N; (void)K;   // (the lists live in registers: only the candidates' copy and the tile boxes)
    return M > 0 ? tiles_of(M) * (KN_TILE * sizeof(float4) + 2 * sizeof(float4)) : 0;
}

int gsr_knn_prepare(int M, const float* candidates, const long long* order, void* workspace, gsr_stream_t stream)
{
    clear_error();
    if (M < 0) return fail_msg("gsr_knn_prepare: negative size");
    if (M == 0) return 0;
    if (!candidates || !order || !workspace) return fail_msg("gsr_knn_prepare: required pointer is null");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail_msg("gsr_knn_prepare: workspace must be 16-byte aligned");
    float4* c4 = static_cast<float4*>(workspace);
    const size_t nt = tiles_of(M);
    knn_prepare_kernel<<<(int)nt, KN_TILE, 0, (hipStream_t)stream>>>(M, candidates, order, c4, c4 + nt * KN_TILE);
    GSR_CHECK_LAUNCH("knn_prepare_kernel");
    return 0;
}

int gsr_knn_search(int N, int M, int K, const float* queries, const long long* query_order, const long long* query_pos,
                   const void* workspace, int exclude_self, int cull, int* idx, float* d2, unsigned long long* stats,
                   gsr_stream_t stream)
{
    clear_error();
    if (N < 0 || M < 0) return fail_msg("gsr_knn_search: negative size");
    if (K < 1 || K > KN_MAX_K) return fail_msg("gsr_knn_search: K must be between 1 and 32");
    if (exclude_self && N != M) return fail_msg("gsr_knn_search: exclude_self needs the queries to be the candidates (N == M)");
    hipStream_t st = (hipStream_t)stream;
    if (stats) GSR_CHECK(hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long), st));
    if (N == 0) return 0;
    if (!queries || !query_order || !idx || !d2 || (M > 0 && !workspace) || (cull && M > 0 && !query_pos))
        return fail_msg("gsr_knn_search: required pointer is null");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail_msg("gsr_knn_search: workspace must be 16-byte aligned");
    const float4* c4 = static_cast<const float4*>(workspace);
    const float4* boxes = c4 + tiles_of(M) * KN_TILE;
    const int grid = blocks(N, KN_QUERIES);
    const int ex = exclude_self != 0, cu = cull != 0 && M > 0;   // (without candidates there is nothing to seed from)
    if (K <= 4)
        knn_search_kernel<4><<<grid, KN_QUERIES, 0, st>>>(N, M, K, queries, query_order, query_pos, c4, boxes, ex, cu, idx, d2, stats);
    else if (K <= 8)
        knn_search_kernel<8><<<grid, KN_QUERIES, 0, st>>>(N, M, K, queries, query_order, query_pos, c4, boxes, ex, cu, idx, d2, stats);
    else if (K <= 16)
        knn_search_kernel<16><<<grid, KN_QUERIES, 0, st>>>(N, M, K, queries, query_order, query_pos, c4, boxes, ex, cu, idx, d2, stats);
    else
        knn_search_kernel<32><<<grid, KN_QUERIES, 0, st>>>(N, M, K, queries, query_order, query_pos, c4, boxes, ex, cu, idx, d2, stats);
    GSR_CHECK_LAUNCH("knn_search_kernel");
    return 0;
}

int gsr_knn_mean_d2(int N, int K, const float* d2, float* out, gsr_stream_t stream)
{
    clear_error();
    if (N < 0) return fail_msg("gsr_knn_mean_d2: negative size");
    if (K < 3) return fail_msg("gsr_knn_mean_d2: rows must hold at least 3 distances");
    if (N == 0) return 0;
    if (!d2 || !out) return fail_msg("gsr_knn_mean_d2: required pointer is null");
    knn_mean_d2_kernel<<<blocks(N, KN_BLOCK), KN_BLOCK, 0, (hipStream_t)stream>>>(N, K, d2, out);
    GSR_CHECK_LAUNCH("knn_mean_d2_kernel");
    return 0;
}

int gsr_knn_segment_mean(int n, int S, int C, const long long* segment_ids, const long long* order, const double* values,
                         double* out, int* count, gsr_stream_t stream)
{
    clear_error();
    if (n < 0 || S < 0 || C < 0) return fail_msg("gsr_knn_segment_mean: negative size");
    if (n == 0 || S == 0) return 0;
    if (!segment_ids || !order || !count || (C > 0 && (!values || !out))) return fail_msg("gsr_knn_segment_mean: required pointer is null");
    knn_segment_mean_kernel<<<blocks(n, KN_BLOCK), KN_BLOCK, 0, (hipStream_t)stream>>>(n, S, C, segment_ids, order, values, out, count);
    GSR_CHECK_LAUNCH("knn_segment_mean_kernel");
    return 0;
}

int gsr_knn_weighted_mean(int N, int K, int C, int M, const int* idx, const float* d2, const double* values, double inv_scale,
                          double* out, gsr_stream_t stream)
{
    clear_error();
    if (N < 0 || C < 0 || M < 0) return fail_msg("gsr_knn_weighted_mean: negative size");
    if (K < 1) return fail_msg("gsr_knn_weighted_mean: K must be positive");
    if (M < 1) return fail_msg("gsr_knn_weighted_mean: needs at least one value row");
    if (N == 0 || C == 0) return 0;
    if (!idx || !d2 || !values || !out) return fail_msg("gsr_knn_weighted_mean: required pointer is null");
    knn_weighted_mean_kernel<<<blocks(N, KN_BLOCK), KN_BLOCK, 0, (hipStream_t)stream>>>(N, K, C, M, idx, d2, values, inv_scale, out);
    GSR_CHECK_LAUNCH("knn_weighted_mean_kernel");
    return 0;
}

}  // extern "C"
