// gsr_density.hip -- the Gaussians' density field: SuGaR's compute_density (gaustar_scene/sugar_model.py:1017-1040, with
// get_covariance(return_full_matrix, return_sqrt, inverse_scales), :619-625), the sum over a point's K nearest Gaussians of
// strength exp(-1/2 Mahalanobis^2): gaustar_amd.density.  The neighbours come from gsr_knn.hip's exact search.
//   records   density_pack_kernel   one 48-byte record per Gaussian, three float4: {cx, cy, cz, strength}, {qr, qi, qj, qk},
//                                   {s0, s1, s2, 0}, the f32 inputs verbatim.  A thread packs four Gaussians: 3 + 3 + 4 + 1
//                                   16-byte loads, 12 16-byte stores; the last P mod 4 go one to a thread by the same stores.
//   field     density_eval_kernel   16 lanes per query, lane j takes neighbour slots j and j + 16, four queries per wave64.  A
//                                   lane reads its neighbour's record with three 16-byte loads and forms the slot's term in
//                                   float64 without contraction, in the order include/gsr.h states; a slot that is empty
//                                   (index -1) or beyond K is +0.0.  A lane adds its two slots, lower first; the 16 lane values
//                                   are summed by the xor butterfly 1, 2, 4, 8 inside the 16-lane row, the same balanced tree in
//                                   every lane.  tests/density_ref.py restates it.
// No LDS, no scratch, no float atomics: a result depends on its own query's row only, so it is the same bits in every call.  The
// one integer atomic is the err word's (bit 0: an index outside [-1, P)).
#include "../../include/gsr.h"
#include "gsr_entry.h"

#include <cstdint>

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int DN_ROW = 16;                        // lanes per query = neighbour slots per pass
constexpr int DN_BLOCK = 256;
constexpr int DN_QUERIES_PER_WAVE = 64 / DN_ROW;
constexpr int DN_QUERIES = DN_BLOCK / DN_ROW;     // per workgroup
constexpr int DN_MAX_K = 2 * DN_ROW;
constexpr int DN_ERR_INDEX = 1;

__global__ void __launch_bounds__(DN_BLOCK) density_pack_kernel(int P, const float* __restrict__ points, const float* __restrict__ scaling,
                                                                const float4* __restrict__ quaternions, const float* __restrict__ strengths,
                                                                float4* __restrict__ records)
{
    const int t = blockIdx.x * DN_BLOCK + threadIdx.x;
    const int groups = P / 4;
    if (t < groups) {
        const float4* p4 = reinterpret_cast<const float4*>(points) + (size_t)3 * t;
        const float4* s4 = reinterpret_cast<const float4*>(scaling) + (size_t)3 * t;
        const float4 pa = p4[0], pb = p4[1], pc = p4[2];
        const float4 sa = s4[0], sb = s4[1], sc = s4[2];
        const float4 w = reinterpret_cast<const float4*>(strengths)[t];
        const float4 q0 = quaternions[(size_t)4 * t], q1 = quaternions[(size_t)4 * t + 1], q2 = quaternions[(size_t)4 * t + 2],
                     q3 = quaternions[(size_t)4 * t + 3];
        float4* r = records + (size_t)12 * t;
        r[0] = make_float4(pa.x, pa.y, pa.z, w.x);   r[1] = q0;   r[2] = make_float4(sa.x, sa.y, sa.z, 0.f);
        r[3] = make_float4(pa.w, pb.x, pb.y, w.y);   r[4] = q1;   r[5] = make_float4(sa.w, sb.x, sb.y, 0.f);
        r[6] = make_float4(pb.z, pb.w, pc.x, w.z);   r[7] = q2;   r[8] = make_float4(sb.z, sb.w, sc.x, 0.f);
        r[9] = make_float4(pc.y, pc.z, pc.w, w.w);   r[10] = q3;  r[11] = make_float4(sc.y, sc.z, sc.w, 0.f);
    } else {
        const int g = 4 * groups + (t - groups);   // (the tail: rows that do not fill a group of four)
        if (g < P) {
            float4* r = records + (size_t)3 * g;
            r[0] = make_float4(points[(size_t)3 * g], points[(size_t)3 * g + 1], points[(size_t)3 * g + 2], strengths[g]);
            r[1] = quaternions[g];
            r[2] = make_float4(scaling[(size_t)3 * g], scaling[(size_t)3 * g + 1], scaling[(size_t)3 * g + 2], 0.f);
        }
    }
}

// one neighbour slot's term: density_factor strength exp(-1/2 m), every operation as include/gsr.h orders it
__device__ __forceinline__ double density_term(double x0, double x1, double x2, float4 c, float4 q, float4 s, double factor)
{
    const double d0 = x0 - (double)c.x, d1 = x1 - (double)c.y, d2 = x2 - (double)c.z;
    const double r = q.x, i = q.y, j = q.z, k = q.w;
    const double two_s = 2.0 / (((r * r + i * i) + j * j) + k * k);
    const double R00 = 1.0 - two_s * (j * j + k * k), R01 = two_s * (i * j - k * r), R02 = two_s * (i * k + j * r);
    const double R10 = two_s * (i * j + k * r), R11 = 1.0 - two_s * (i * i + k * k), R12 = two_s * (j * k - i * r);
    const double R20 = two_s * (i * k - j * r), R21 = two_s * (j * k + i * r), R22 = 1.0 - two_s * (i * i + j * j);
    const double s0 = s.x, s1 = s.y, s2 = s.z;
    const double inv0 = 1.0 / (s0 < 1e-8 ? 1e-8 : s0), inv1 = 1.0 / (s1 < 1e-8 ? 1e-8 : s1), inv2 = 1.0 / (s2 < 1e-8 ? 1e-8 : s2);
    const double w0 = inv0 * ((R00 * d0 + R10 * d1) + R20 * d2);
    const double w1 = inv1 * ((R01 * d0 + R11 * d1) + R21 * d2);
    const double w2 = inv2 * ((R02 * d0 + R12 * d1) + R22 * d2);
    double m = (w0 * w0 + w1 * w1) + w2 * w2;
    m = m < 0.0 ? 0.0 : (m > 1e8 ? 1e8 : m);   // (:1033's clamp as selects: a NaN stays)
    return (factor * (double)c.w) * exp(-0.5 * m);
}

__global__ void __launch_bounds__(DN_BLOCK) density_eval_kernel(int Q, int P, int K, const float* __restrict__ x, const int* __restrict__ idx,
                                                                const float4* __restrict__ records, float density_factor,
                                                                float* __restrict__ density, float* __restrict__ opacities,
                                                                int* __restrict__ err)
{
    const int lane = threadIdx.x & (DN_ROW - 1);
    const long long ql = (long long)blockIdx.x * DN_QUERIES + (threadIdx.x / DN_ROW);
    const bool live = ql < Q;
    const size_t q = live ? (size_t)ql : 0;
    const double x0 = x[3 * q], x1 = x[3 * q + 1], x2 = x[3 * q + 2];
    const double factor = (double)density_factor;
    double t[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int slot = lane + h * DN_ROW;
        t[h] = 0.0;
        if (live && slot < K) {
            const int id = idx[q * K + slot];
            if ((unsigned)id < (unsigned)P) {
                const float4* r = records + (size_t)3 * id;
                t[h] = density_term(x0, x1, x2, r[0], r[1], r[2], factor);
            } else if (id != -1) {
                atomicOr(err, DN_ERR_INDEX);
            }
            if (opacities) opacities[q * K + slot] = (float)t[h];
        }
    }
    double v = t[0] + t[1];
#pragma unroll
    for (int m = 1; m < DN_ROW; m <<= 1) v = v + __shfl_xor(v, m, DN_ROW);
    if (live && lane == 0) density[q] = (float)v;
}

inline int blocks(long long n, int b) { return (int)((n + b - 1) / b); }

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

int gsr_density_queries_per_wave(void) { return DN_QUERIES_PER_WAVE; }
int gsr_density_queries_per_workgroup(void) { return DN_QUERIES; }

int gsr_density_pack(int P, const float* points, const float* scaling, const float* quaternions, const float* strengths, void* records,
                     gsr_stream_t stream)
{
    clear_error();
    if (P < 0) return fail_msg("gsr_density_pack: negative size");
    if (P == 0) return 0;
    if (!points || !scaling || !quaternions || !strengths || !records) return fail_msg("gsr_density_pack: required pointer is null");
    if ((reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(scaling) | reinterpret_cast<uintptr_t>(quaternions) |
         reinterpret_cast<uintptr_t>(strengths) | reinterpret_cast<uintptr_t>(records)) & 15)
        return fail_msg("gsr_density_pack: every array must be 16-byte aligned");
    const int threads = P / 4 + P % 4;
    density_pack_kernel<<<blocks(threads, DN_BLOCK), DN_BLOCK, 0, (hipStream_t)stream>>>(
        P, points, scaling, reinterpret_cast<const float4*>(quaternions), strengths, static_cast<float4*>(records));
    GSR_CHECK_LAUNCH("density_pack_kernel");
    return 0;
}

int gsr_density_eval(int Q, int P, int K, const float* x, const int* idx, const void* records, float density_factor, float* density,
                     float* neighbor_opacities, int* err, gsr_stream_t stream)
{
    clear_error();
    if (Q < 0 || P < 0) return fail_msg("gsr_density_eval: negative size");
    if (K < 1 || K > DN_MAX_K) return fail_msg("gsr_density_eval: K must be between 1 and 32");
    if (Q == 0) return 0;
    if (P < 1) return fail_msg("gsr_density_eval: needs at least one Gaussian");
    if (!x || !idx || !records || !density || !err) return fail_msg("gsr_density_eval: required pointer is null");
    if (reinterpret_cast<uintptr_t>(records) & 15) return fail_msg("gsr_density_eval: records must be 16-byte aligned");
    density_eval_kernel<<<blocks(Q, DN_QUERIES), DN_BLOCK, 0, (hipStream_t)stream>>>(
        Q, P, K, x, idx, static_cast<const float4*>(records), density_factor, density, neighbor_opacities, err);
    GSR_CHECK_LAUNCH("density_eval_kernel");
    return 0;
}

}  // extern "C"
