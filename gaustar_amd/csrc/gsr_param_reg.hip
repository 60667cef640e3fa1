// gsr_param_reg.hip -- the regularisers of a refinement iteration that live on the Gaussians' own parameters, fused: the two
// loose-bind penalties, the opacity floor and the SH (dc) regulariser (gaustar_trainers/refine.py:739-740, :743-748, :663-669):
//   loose_t = factor_t * (w * |delta_t|).mean()             over 3N elements
//   loose_r = factor_r * (w * |delta_r[:, 1:]|).mean()      over 3N elements
//   opacity = relu(min_opacity - sigmoid(densities)).mean() over N
//   sh      = sh_factor * ((pre_sh_dc - sh_dc[:M]) ** 2).mean() over 3M
// A pure streaming op.  A thread takes PR_G = 4 consecutive Gaussians, so every array is read and written as whole 16-byte
// words (the 12-byte rows of delta_t / sh_dc as the flat 3N array they are: 4 rows = 3 float4); a scalar path serves the
// ragged last group and arrays that are not 16-byte aligned.
//   forward   one element pass and one single-workgroup finalise, summed in double in a fixed order (gsr_reduce.h)
//             -> loss_out[5] = {loose_t, loose_r, opacity, sh, total};
//   backward  elementwise; no float atomics anywhere: two calls give identical bits.
// Gradients at the kinks follow torch: d|x|/dx = 0 at 0 (delta_t starts at exactly 0), relu'(0) = 0; delta_r[:, 0] and the
// sh_dc rows at or beyond M get exactly 0.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_reduce.h"
#include <cstdio>

namespace gsr {

namespace {

constexpr int PR_BLOCK = RED_BLOCK;  // forward and backward walk the groups with the same grid
constexpr int PR_G = 4;             // Gaussians per thread

struct ParamRegArgs {
    int N, M;
    const float* delta_t;     // [N,3] or null
    const float* delta_r;     // [N,4] (w first) or null
    const float* weight;      // element (n, c) at weight[n * w_rs + c * w_cs]; null: 1
    long long w_rs, w_cs;
    const float* densities;   // [N] raw or null
    const float* sh_dc;       // [N,3] or null
    const float* pre_sh_dc;   // [M,3] or null
    float min_opacity;
    int use_t, use_r, use_o, use_sh;
    int vec;                  // every array given is 16-byte aligned
};

// K floats per Gaussian of the group starting at Gaussian g0 with cnt (1..4) rows; rows beyond cnt read as 0
template <int K>
__device__ __forceinline__ void ld_group(const float* __restrict__ p, int g0, int cnt, int vec, float (&v)[PR_G * K])
{
    const float* q = p + (size_t)g0 * K;
    if (vec && cnt == PR_G) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            const float4 t = reinterpret_cast<const float4*>(q)[j];
            v[4 * j] = t.x; v[4 * j + 1] = t.y; v[4 * j + 2] = t.z; v[4 * j + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < PR_G * K; i++) v[i] = i < cnt * K ? q[i] : 0.f;
    }
}

// the same group written (acc = 0) or added to what is there with one rounding per element (acc = 1: torch's X + fresh)
template <int K>
__device__ __forceinline__ void st_group(float* __restrict__ p, int g0, int cnt, int vec, int acc, const float (&v)[PR_G * K])
{
#pragma clang fp contract(off)
    float* q = p + (size_t)g0 * K;
    if (vec && cnt == PR_G) {
#pragma unroll
        for (int j = 0; j < K; j++) {
            float4 t = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
            if (acc) {
                const float4 o = reinterpret_cast<const float4*>(q)[j];
                t.x = o.x + t.x; t.y = o.y + t.y; t.z = o.z + t.z; t.w = o.w + t.w;
            }
            reinterpret_cast<float4*>(q)[j] = t;
        }
    } else {
#pragma unroll
        for (int i = 0; i < PR_G * K; i++)
            if (i < cnt * K) q[i] = acc ? q[i] + v[i] : v[i];
    }
}

// weights of the group's rows: w[3 * i + c] = weight of Gaussian g0 + i, axis c (rows beyond cnt: 0)
__device__ __forceinline__ void ld_weights(const ParamRegArgs& a, int g0, int cnt, float (&w)[PR_G * 3])
{
#pragma unroll
    for (int i = 0; i < PR_G; i++) {
        if (a.weight == nullptr || i >= cnt) {
            const float one = i < cnt ? 1.f : 0.f;
            w[3 * i] = one; w[3 * i + 1] = one; w[3 * i + 2] = one;
        } else {
            const float* r = a.weight + (long long)(g0 + i) * a.w_rs;
            const float w0 = r[0];
            w[3 * i] = w0;
            w[3 * i + 1] = a.w_cs ? r[a.w_cs] : w0;        // (column stride 0: a [N] tensor or an expanded view, one load)
            w[3 * i + 2] = a.w_cs ? r[2 * a.w_cs] : w0;
        }
    }
}

// torch.sigmoid as gsr_sh_colors_split evaluates it: the Gaussians the opacity term pushes are those rendered below the floor
__device__ __forceinline__ float sigmoidf(float d) { return 1.0f / (1.0f + expf(-d)); }

__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : x < 0.f ? -1.f : 0.f; }   // torch.sign: 0 at 0

__global__ void __launch_bounds__(PR_BLOCK)
param_reg_fwd_kernel(ParamRegArgs a, double* __restrict__ partials)
{
    const int n_groups = (a.N + PR_G - 1) / PR_G;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int g = (int)(blockIdx.x * PR_BLOCK + threadIdx.x); g < n_groups; g += (int)(gridDim.x * PR_BLOCK)) {
        const int g0 = g * PR_G, cnt = min(PR_G, a.N - g0);
        float w[PR_G * 3];
        if (a.use_t || a.use_r) ld_weights(a, g0, cnt, w);
        if (a.use_t) {
            float v[PR_G * 3];
            ld_group<3>(a.delta_t, g0, cnt, a.vec, v);
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < PR_G * 3; i++) t += w[i] * fabsf(v[i]);
            s[0] += (double)t;
        }
        if (a.use_r) {
            float v[PR_G * 4];
            ld_group<4>(a.delta_r, g0, cnt, a.vec, v);
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < PR_G; i++) {
#pragma unroll
                for (int c = 0; c < 3; c++) t += w[3 * i + c] * fabsf(v[4 * i + 1 + c]);
            }
            s[1] += (double)t;
        }
        if (a.use_o) {
            float v[PR_G];
            ld_group<1>(a.densities, g0, cnt, a.vec, v);
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < PR_G; i++)
                if (i < cnt) t += fmaxf(a.min_opacity - sigmoidf(v[i]), 0.f);
            s[2] += (double)t;
        }
        const int cm = min(PR_G, a.M - g0);     // rows of this group inside the tracked prefix
        if (a.use_sh && cm > 0) {
            float v[PR_G * 3], p[PR_G * 3];
            ld_group<3>(a.sh_dc, g0, cm, a.vec, v);
            ld_group<3>(a.pre_sh_dc, g0, cm, a.vec, p);
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < PR_G * 3; i++) { const float d = p[i] - v[i]; t += d * d; }
            s[3] += (double)t;
        }
    }
    block_partials(s, partials);
}

__global__ void __launch_bounds__(PR_BLOCK)
param_reg_finalize_kernel(int n_wg, const double* __restrict__ partials, ParamRegArgs a, float factor_t, float factor_r,
                          float sh_factor, float* __restrict__ out)
{
    double r[4];   // (defined in thread 0 only)
    tree_total(n_wg, partials, r);
    if (threadIdx.x == 0) {
        const double n3 = 3.0 * (double)a.N, m3 = 3.0 * (double)a.M;
        const float lt = a.use_t ? (float)((double)factor_t * (r[0] / n3)) : 0.f;
        const float lr = a.use_r ? (float)((double)factor_r * (r[1] / n3)) : 0.f;
        const float op = a.use_o ? (float)(r[2] / (double)a.N) : 0.f;
        const float sh = a.use_sh ? (float)((double)sh_factor * (r[3] / m3)) : 0.f;
        out[0] = lt; out[1] = lr; out[2] = op; out[3] = sh;
        out[4] = ((lt + lr) + op) + sh;
    }
}

struct ParamRegGrads {
    float* d_t;      // [N,3]
    float* d_r;      // [N,4]
    float* d_dens;   // [N]
    float* d_sh;     // [N,3]
    float ct, cr, co, csh;   // factor_t / 3N, factor_r / 3N, 1 / N, 2 sh_factor / 3M
};

__global__ void __launch_bounds__(PR_BLOCK)
param_reg_bwd_kernel(ParamRegArgs a, ParamRegGrads o, const float* __restrict__ scale, int accumulate)
{
    // never contracted: a fresh value is the same product chain whether it is written or added
#pragma clang fp contract(off)
    const int n_groups = (a.N + PR_G - 1) / PR_G;
    const float s = scale ? *scale : 1.f;
    for (int g = (int)(blockIdx.x * PR_BLOCK + threadIdx.x); g < n_groups; g += (int)(gridDim.x * PR_BLOCK)) {
        const int g0 = g * PR_G, cnt = min(PR_G, a.N - g0);
        float w[PR_G * 3];
        if (o.d_t || o.d_r) ld_weights(a, g0, cnt, w);
        if (o.d_t) {
            float v[PR_G * 3], gr[PR_G * 3];
            ld_group<3>(a.delta_t, g0, cnt, a.vec, v);
            const float k = s * o.ct;
#pragma unroll
            for (int i = 0; i < PR_G * 3; i++) gr[i] = (k * w[i]) * sgn(v[i]);
            st_group<3>(o.d_t, g0, cnt, a.vec, accumulate, gr);
        }
        if (o.d_r) {
            float v[PR_G * 4], gr[PR_G * 4];
            ld_group<4>(a.delta_r, g0, cnt, a.vec, v);
            const float k = s * o.cr;
#pragma unroll
            for (int i = 0; i < PR_G; i++) {
                gr[4 * i] = 0.f;
#pragma unroll
                for (int c = 0; c < 3; c++) gr[4 * i + 1 + c] = (k * w[3 * i + c]) * sgn(v[4 * i + 1 + c]);
            }
            st_group<4>(o.d_r, g0, cnt, a.vec, accumulate, gr);
        }
        if (o.d_dens) {
            float v[PR_G], gr[PR_G];
            ld_group<1>(a.densities, g0, cnt, a.vec, v);
            const float k = -(s * o.co);
#pragma unroll
            for (int i = 0; i < PR_G; i++) {
                const float op = sigmoidf(v[i]);
                gr[i] = a.min_opacity - op > 0.f ? k * ((1.f - op) * op) : 0.f;    // relu'(0) = 0; sigmoid_backward
            }
            st_group<1>(o.d_dens, g0, cnt, a.vec, accumulate, gr);
        }
        if (o.d_sh) {
            const int cm = max(0, min(PR_G, a.M - g0));
            float v[PR_G * 3], p[PR_G * 3], gr[PR_G * 3];
            if (cm > 0) {
                ld_group<3>(a.sh_dc, g0, cm, a.vec, v);
                ld_group<3>(a.pre_sh_dc, g0, cm, a.vec, p);
            }
            const float k = s * o.csh;
#pragma unroll
            for (int i = 0; i < PR_G * 3; i++) gr[i] = i < cm * 3 ? k * (v[i] - p[i]) : 0.f;
            st_group<3>(o.d_sh, g0, cnt, a.vec, accumulate, gr);
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

ParamRegArgs make_args(int N, int M, const float* delta_t, const float* delta_r, const float* weight, long long w_rs,
                       long long w_cs, float factor_t, float factor_r, const float* densities, float min_opacity,
                       const float* sh_dc, const float* pre_sh_dc, float sh_factor)
{
    ParamRegArgs a{};
    a.N = N; a.M = M; a.delta_t = delta_t; a.delta_r = delta_r; a.weight = weight; a.w_rs = w_rs; a.w_cs = w_cs;
    a.densities = densities; a.sh_dc = sh_dc; a.pre_sh_dc = pre_sh_dc; a.min_opacity = min_opacity;
    a.use_t = N > 0 && delta_t != nullptr && factor_t != 0.f;
    a.use_r = N > 0 && delta_r != nullptr && factor_r != 0.f;
    a.use_o = N > 0 && densities != nullptr;
    a.use_sh = M > 0 && sh_dc != nullptr && pre_sh_dc != nullptr && sh_factor != 0.f;
    a.vec = aligned16(delta_t) && aligned16(delta_r) && aligned16(densities) && aligned16(sh_dc) && aligned16(pre_sh_dc);
    return a;
}

int n_workgroups(int N) { return reduce_workgroups(((long long)N + PR_G - 1) / PR_G); }   // (PR_BLOCK lanes each take a group)

// gsr_param_reg_backward's launch: a skipped term touches no gradient buffer
void launch_param_reg_grad(ParamRegArgs a, float factor_t, float factor_r, float sh_factor, const float* scale, float* d_delta_t,
                           float* d_delta_r, float* d_densities, float* d_sh_dc, int accumulate, hipStream_t st)
{
    ParamRegGrads o{};
    o.d_t = a.use_t ? d_delta_t : nullptr;
    o.d_r = a.use_r ? d_delta_r : nullptr;
    o.d_dens = a.use_o ? d_densities : nullptr;
    o.d_sh = a.use_sh ? d_sh_dc : nullptr;
    if (!o.d_t && !o.d_r && !o.d_dens && !o.d_sh) return;
    a.vec = a.vec && aligned16(o.d_t) && aligned16(o.d_r) && aligned16(o.d_dens) && aligned16(o.d_sh);
    o.ct = a.use_t ? (float)((double)factor_t / (3.0 * (double)a.N)) : 0.f;
    o.cr = a.use_r ? (float)((double)factor_r / (3.0 * (double)a.N)) : 0.f;
    o.co = a.use_o ? (float)(1.0 / (double)a.N) : 0.f;
    o.csh = a.use_sh ? (float)(2.0 * (double)sh_factor / (3.0 * (double)a.M)) : 0.f;
    param_reg_bwd_kernel<<<n_workgroups(a.N), PR_BLOCK, 0, st>>>(a, o, scale, accumulate);
}

int param_reg_check(const char* fn, int N, int M, const float* weight, long long w_rs, long long w_cs)
{
    char msg[160];
    if (N < 0 || M < 0 || M > N) { snprintf(msg, sizeof msg, "%s: need 0 <= M <= N", fn); return fail_msg(msg); }
    if (N >= (1 << 29)) { snprintf(msg, sizeof msg, "%s: too many Gaussians", fn); return fail_msg(msg); }
    if (weight && (w_rs < 0 || w_cs < 0)) { snprintf(msg, sizeof msg, "%s: negative weight stride", fn); return fail_msg(msg); }
    return 0;
}

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

size_t gsr_param_reg_workspace_bytes(int N)
{
    (void)N;   // (the partials of at most 2048 workgroups, whatever the model)
    return reduce_workspace_bytes();
}

int gsr_param_reg_forward(int N, int M, const float* delta_t, const float* delta_r, const float* weight, long long w_row_stride,
                          long long w_col_stride, float factor_t, float factor_r, const float* densities, float min_opacity,
                          const float* sh_dc, const float* pre_sh_dc, float sh_factor, void* workspace, float* loss_out,
                          gsr_stream_t stream)
{
    clear_error();
    if (int rc = param_reg_check("gsr_param_reg_forward", N, M, weight, w_row_stride, w_col_stride)) return rc;
    if (!workspace || !loss_out) return fail_msg("gsr_param_reg_forward: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    {
        Scope sc(ST_LOSS, st);
        const ParamRegArgs a = make_args(N, M, delta_t, delta_r, weight, w_row_stride, w_col_stride, factor_t, factor_r, densities,
                                         min_opacity, sh_dc, pre_sh_dc, sh_factor);
        double* partials = static_cast<double*>(workspace);
        const int n_wg = (a.use_t || a.use_r || a.use_o || a.use_sh) ? n_workgroups(N) : 0;
        if (n_wg > 0) param_reg_fwd_kernel<<<n_wg, PR_BLOCK, 0, st>>>(a, partials);
        param_reg_finalize_kernel<<<1, PR_BLOCK, 0, st>>>(n_wg, partials, a, factor_t, factor_r, sh_factor, loss_out);
    }
    GSR_CHECK_LAUNCH("param_reg forward kernels");
    return 0;
}

int gsr_param_reg_backward(int N, int M, const float* delta_t, const float* delta_r, const float* weight, long long w_row_stride,
                           long long w_col_stride, float factor_t, float factor_r, const float* densities, float min_opacity,
                           const float* sh_dc, const float* pre_sh_dc, float sh_factor, const float* grad_scale,
                           float* dL_ddelta_t, float* dL_ddelta_r, float* dL_ddensities, float* dL_dsh_dc, int accumulate,
                           gsr_stream_t stream)
{
    clear_error();
    if (int rc = param_reg_check("gsr_param_reg_backward", N, M, weight, w_row_stride, w_col_stride)) return rc;
    if (accumulate != 0 && accumulate != 1) return fail_msg("gsr_param_reg_backward: accumulate must be 0 or 1");
    if (N == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    {
        Scope sc(ST_LOSS, st);
        launch_param_reg_grad(make_args(N, M, delta_t, delta_r, weight, w_row_stride, w_col_stride, factor_t, factor_r, densities,
                                        min_opacity, sh_dc, pre_sh_dc, sh_factor),
                              factor_t, factor_r, sh_factor, grad_scale, dL_ddelta_t, dL_ddelta_r, dL_ddensities, dL_dsh_dc, accumulate,
                              st);
    }
    GSR_CHECK_LAUNCH("param_reg_bwd_kernel");
    return 0;
}

}  // extern "C"
