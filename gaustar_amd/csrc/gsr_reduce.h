// gsr_reduce.h -- the deterministic f64 sum of the fused regularisers (gsr_mesh_reg.hip, gsr_param_reg.hip): K sums per
// workgroup of an element pass, then one workgroup that adds the partials in a fixed order.  No float atomics: two calls give
// identical bits.
#pragma once
#include "gsr_internal.h"

namespace gsr {

namespace {

constexpr int RED_BLOCK = 256;      // workgroup of the element pass and of the finalise
constexpr int RED_MAX_WGS = 2048;   // element pass: grid-stride beyond 2048 workgroups
constexpr int RED_STRIDE = 4;       // doubles per workgroup in the partials, whatever K <= 4

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// s[0 .. K) of every lane of the workgroup -> partials[RED_STRIDE blockIdx.x + k]: a shuffle tree per wave, then the waves
// in order
template <int K>
__device__ __forceinline__ void block_partials(double (&s)[K], double* __restrict__ partials)
{
    static_assert(K <= RED_STRIDE, "a workgroup's partials hold RED_STRIDE sums");
    __shared__ double red[RED_BLOCK / 64][K];
#pragma unroll
    for (int k = 0; k < K; k++) s[k] = wave_sum(s[k]);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[wv][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < RED_BLOCK / 64; w++) t += red[w][threadIdx.x];
        partials[RED_STRIDE * blockIdx.x + threadIdx.x] = t;
    }
}

// the K totals over n_wg workgroups' partials, by one workgroup of RED_BLOCK lanes: a strided f64 accumulation per lane, then
// the fixed-order tree in LDS.  Thread 0 alone gets the totals.
template <int K>
__device__ __forceinline__ void tree_total(int n_wg, const double* __restrict__ partials, double (&total)[K])
{
    __shared__ double r[K][RED_BLOCK];
    double v[K];
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = 0.0;
    for (int i = threadIdx.x; i < n_wg; i += RED_BLOCK) {
#pragma unroll
        for (int k = 0; k < K; k++) v[k] += partials[RED_STRIDE * i + k];
    }
#pragma unroll
    for (int k = 0; k < K; k++) r[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int d = RED_BLOCK / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
#pragma unroll
            for (int k = 0; k < K; k++) r[k][threadIdx.x] += r[k][threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) total[k] = r[k][0];
    }
}

// the grid of an element pass over n elements: a workgroup per RED_BLOCK of them, grid-stride beyond RED_MAX_WGS (0 for n = 0)
inline int reduce_workgroups(long long n)
{
    const long long wg = (n + RED_BLOCK - 1) / RED_BLOCK;
    return (int)(wg < RED_MAX_WGS ? wg : RED_MAX_WGS);
}

inline size_t reduce_workspace_bytes() { return align_up(RED_STRIDE * sizeof(double) * RED_MAX_WGS) + 256; }

}  // namespace

}  // namespace gsr
