// gsr_flow.hip -- RAFT optical flow (the basic model, inference): the kernels gaustar_amd.flow strings together, replacing the
// reference's data_process/RAFT (core/raft.py, corr.py, update.py, extractor.py, utils/utils.py, demo_GauSTAR.py).
// All activations are f32, NHWC.  A buffer may be a channel slice of a wider one (FlowSlice: base, floats per pixel, first
// channel, channels), so the reference's torch.cat's of [h, x], [r*h, x], [inp, motion], [cor, flo] and [out, flow] are
// buffers that two convolutions write side by side and cost nothing.
//   flow_prep_kernel      u8 [h,w,3] -> f32 [Hp,Wp,3]: box mean over factor x factor (integers, half to even, as cvRound), replicate
//                         padding to a multiple of 8 split pad//2 before (InputPadder, 'sintel'), then 2 (x / 255) - 1.
//   flow_conv_kernel      convolution as implicit GEMM on v_mfma_f32_32x32x2_f32: M = N Ho Wo output pixels, N = Cout, K = KH KW
//                         Cin in (ky, kx, ci) order.  A workgroup of four waves makes a 64 x 64 tile, a wave a 32 x 32 quarter
//                         of it (16 accumulator registers); K advances 16 at a time through LDS ([k][m] and [k][n] images with
//                         96-float rows: the two halves of a wave read different banks; two images, one barrier a step), the
//                         global loads of two steps ahead in flight while the current one multiplies.  An output is one k-ordered f32 fma chain from 0.  Weights are
//                         packed once as [Kpad][Npad] (zeros beyond K and Cout), so the B loader has no bounds.  The A loader
//                         reads 16 bytes where every slice is 4-channel aligned and falls back to scalars (Cin = 2, 3, the
//                         flow's 2 channels at the end of a 128-wide buffer).  Epilogue: alpha, bias, per-channel scale and
//                         shift (eval-mode batch norm, after the bias), activation, residual add (+ relu), channel-offset store.
//                         The correlation volume is the same kernel: its "weights" are the other feature map, packed by
//                         flow_pack_kernel, alpha = 1 / sqrt(256).
//   flow_conv_thin_kernel Cout <= 4 (the flow head's 2): one wave per output pixel, lane-strided fma chains joined by a fixed
//                         shuffle tree; the same loader and epilogue.
//   flow_in_*             instance norm per (image, channel) over H W, biased variance, eps 1e-5, no affine: f64 sums per
//                         256-pixel chunk in a fixed order, gsr_reduce.h's tree over the chunks, then (x - mean) rstd (+ relu)
//                         (+ residual, relu).  Images never mix: the chunk grid has the image as its second axis.
//   flow_pool_kernel      2 x 2 mean over the last two axes of a volume level, odd sizes floored.
//   flow_lookup_kernel    per feature pixel and level l: the 9 x 9 window around (grid + flow) / 2^l, bilinear, zero outside;
//                         channel l 81 + i 9 + j samples at (x + d_i, y + d_j) (corr.py:37-43 stacks (dy, dx) onto (x, y)).
//   flow_gru_kernel       r h, and h <- (1 - z) h + z q; 16-byte accesses.
//   flow_upsample_kernel  softmax over the 9 logits 0.25 mask, weighted sum of the 3 x 3 neighbourhood of 8 flow (zero padded),
//                         8 x upsampled, unpadded, [h,w,2] in (x, y) order.
// No atomics of any kind, no scratch; every output is a pure function of the inputs with a fixed order of operations.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_reduce.h"

#include <cstddef>
#include <cstdint>
#include <string>

namespace gsr {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int FC_BM = 64, FC_BN = 64, FC_BK = 16, FC_LD = 96, FC_THREADS = 256;
constexpr int FC_THIN = 4;      // Cout up to this takes the one-wave-per-pixel kernel (its float4 of weights per row)
constexpr int FLOW_LEVELS = 4, FLOW_RADIUS = 4, FLOW_WIN = 2 * FLOW_RADIUS + 1, FLOW_CORR_CH = FLOW_LEVELS * FLOW_WIN * FLOW_WIN;
constexpr int FLOW_MASK_CH = 576;
constexpr int IN_CHUNK = 256;     // pixels per workgroup of the instance norm's sums

struct FlowSlice { const float* base; long long stride; int off; int ch; };   // = gsr_flow_slice

struct ConvArgs {
    int N, H, W, Ho, Wo, KH, KW, S, PH, PW;
    int Cin, K, Cout, Npad, n_in;
    long long M;
    FlowSlice in[3];
    const float *w, *bias, *scale, *shift;
    float alpha;
    int act;
    float* out; long long out_stride; int out_off;
    const float* res; long long res_stride; int res_off; int res_relu;
};

__device__ __forceinline__ const float* slice_ptr(const ConvArgs& a, long long pix, int ci)
{
    if (ci < a.in[0].ch) return a.in[0].base + pix * a.in[0].stride + a.in[0].off + ci;
    ci -= a.in[0].ch;
    if (ci < a.in[1].ch) return a.in[1].base + pix * a.in[1].stride + a.in[1].off + ci;
    ci -= a.in[1].ch;
    return a.in[2].base + pix * a.in[2].stride + a.in[2].off + ci;
}

__device__ __forceinline__ float activate(float v, int act)
{
    if (act == 1) return fmaxf(v, 0.0f);
    if (act == 2) return 1.0f / (1.0f + expf(-v));
    if (act == 3) return tanhf(v);
    return v;
}

struct PixelAt { bool valid; int img, iy0, ix0; };

__device__ __forceinline__ PixelAt pixel_at(const ConvArgs& a, long long m)
{
    PixelAt p = {m < a.M, 0, 0, 0};
    if (p.valid) {
        const int hw = a.Ho * a.Wo;
        p.img = (int)(m / hw);
        const int rem = (int)(m - (long long)p.img * hw);
        const int oy = rem / a.Wo, ox = rem - oy * a.Wo;
        p.iy0 = oy * a.S - a.PH;
        p.ix0 = ox * a.S - a.PW;
    }
    return p;
}

// the inputs of k = kb .. kb + 3 (kb a multiple of 4) at output pixel p: zeros beyond K, outside the image and for an invalid pixel
template <bool VEC>
__device__ __forceinline__ void load_k4(const ConvArgs& a, const PixelAt& p, int kb, float (&r)[4])
{
    r[0] = r[1] = r[2] = r[3] = 0.0f;
    if (!p.valid) return;
    if (VEC) {
        if (kb >= a.K) return;
        const int tap = kb / a.Cin, ci = kb - tap * a.Cin;
        const int ky = tap / a.KW, kx = tap - ky * a.KW;
        const int iy = p.iy0 + ky, ix = p.ix0 + kx;
        if (iy < 0 || iy >= a.H || ix < 0 || ix >= a.W) return;
        const long long pix = ((long long)p.img * a.H + iy) * a.W + ix;
        const float4 v = *reinterpret_cast<const float4*>(slice_ptr(a, pix, ci));
        r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = kb + j;
            if (k >= a.K) continue;
            const int tap = k / a.Cin, ci = k - tap * a.Cin;
            const int ky = tap / a.KW, kx = tap - ky * a.KW;
            const int iy = p.iy0 + ky, ix = p.ix0 + kx;
            if (iy < 0 || iy >= a.H || ix < 0 || ix >= a.W) continue;
            const long long pix = ((long long)p.img * a.H + iy) * a.W + ix;
            r[j] = *slice_ptr(a, pix, ci);
        }
    }
}

struct ColumnTail { float bias, sc, sh; bool affine; };

__device__ __forceinline__ ColumnTail column_tail(const ConvArgs& a, int col)
{
    ColumnTail t;
    t.bias = a.bias ? a.bias[col] : 0.0f;
    t.affine = a.scale != nullptr;
    t.sc = t.affine ? a.scale[col] : 1.0f;
    t.sh = t.affine ? a.shift[col] : 0.0f;
    return t;
}

__device__ __forceinline__ void store_out(const ConvArgs& a, const ColumnTail& t, long long row, int col, float sum)
{
    float v = sum * a.alpha + t.bias;
    if (t.affine) v = v * t.sc + t.sh;
    v = activate(v, a.act);
    if (a.res) {
        v += a.res[row * a.res_stride + a.res_off + col];
        if (a.res_relu) v = fmaxf(v, 0.0f);
    }
    a.out[row * a.out_stride + a.out_off + col] = v;
}

template <bool VEC>
__global__ __launch_bounds__(FC_THREADS) void flow_conv_kernel(const ConvArgs a)
{
    __shared__ __attribute__((aligned(16))) float As[2][FC_BK][FC_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][FC_BK][FC_LD];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const long long m0 = (long long)blockIdx.x * FC_BM;
    const int n0 = blockIdx.y * FC_BN;

    // A loader: pixel m0 + (t & 63), the four k of quad (t >> 6) of the step;  B loader: row t >> 4 of the step, columns 4 (t & 15) ..
    const int am = t & 63, akq = t >> 6;
    const PixelAt px = pixel_at(a, m0 + am);
    const int bk = t >> 4, bn = (t & 15) * 4;
    const int nk = (a.K + FC_BK - 1) / FC_BK;
    const int wm = (wv & 1) * 32, wn = (wv >> 1) * 32;

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.0f;

    auto load_step = [&](int kt, float (&ra)[4], float4& rb) {
        load_k4<VEC>(a, px, kt * FC_BK + akq * 4, ra);
        rb = *reinterpret_cast<const float4*>(a.w + (long long)(kt * FC_BK + bk) * a.Npad + n0 + bn);
    };
    // one step: the registers loaded two steps ago go to LDS image `buf`, the loads of step kt + 2 start, the image multiplies.
    // One barrier a step: a wave writes image `buf` again only after the barrier of the step between, which every wave
    // reaches after it has read `buf`.
    auto step = [&](int kt, int buf, float (&ra)[4], float4& rb) {
#pragma unroll
        for (int j = 0; j < 4; j++) As[buf][akq * 4 + j][am] = ra[j];
        *reinterpret_cast<float4*>(&Bs[buf][bk][bn]) = rb;
        __syncthreads();
        if (kt + 2 < nk) load_step(kt + 2, ra, rb);
#pragma unroll
        for (int kk = 0; kk < FC_BK; kk += 2) {
            const float av = As[buf][kk + (lane >> 5)][wm + (lane & 31)];
            const float bv = Bs[buf][kk + (lane >> 5)][wn + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
    };
    float ra0[4], ra1[4];
    float4 rb0, rb1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    load_step(0, ra0, rb0);
    if (nk > 1) load_step(1, ra1, rb1);
    for (int kt = 0; kt < nk; kt += 2) {
        step(kt, 0, ra0, rb0);
        if (kt + 1 < nk) step(kt + 1, 1, ra1, rb1);
    }

    // epilogue: the lane holds column wn + (lane & 31) and rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of its wave's quarter
    const int col = n0 + wn + (lane & 31);
    if (col >= a.Cout) return;
    const ColumnTail tail = column_tail(a, col);
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const long long row = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row < a.M) store_out(a, tail, row, col, acc[r]);
    }
}

// Cout <= FC_THIN (the flow head's two channels): a 64-wide tile of the matrix kernel would be 1/32 full.  One wave per output
// pixel; lane l takes k = 4 l .. 4 l + 3, + 256, ...: per channel a k-ordered fma chain per lane, the 64 chains joined by a
// fixed shuffle tree.  Same loader, same epilogue.
template <bool VEC>
__global__ __launch_bounds__(256) void flow_conv_thin_kernel(const ConvArgs a)
{
    const int lane = threadIdx.x & 63;
    const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= a.M) return;                                     // wave-uniform
    const PixelAt px = pixel_at(a, m);
    float acc[FC_THIN];
#pragma unroll
    for (int c = 0; c < FC_THIN; c++) acc[c] = 0.0f;
#pragma unroll 3
    for (int kb = lane * 4; kb < a.K; kb += 256) {            // rows kb .. kb + 3 of the packed weights exist: Kpad is a multiple of 16
        float r[4];
        load_k4<VEC>(a, px, kb, r);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float4 w = *reinterpret_cast<const float4*>(a.w + (long long)(kb + j) * a.Npad);      // columns beyond Cout hold zeros
            acc[0] = fmaf(r[j], w.x, acc[0]);
            acc[1] = fmaf(r[j], w.y, acc[1]);
            acc[2] = fmaf(r[j], w.z, acc[2]);
            acc[3] = fmaf(r[j], w.w, acc[3]);
        }
    }
    float mine = 0.0f;
#pragma unroll
    for (int c = 0; c < FC_THIN; c++) {
        float v = acc[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        v = __shfl(v, 0, 64);
        if (lane == c) mine = v;
    }
    if (lane < a.Cout) store_out(a, column_tail(a, lane), m, lane, mine);
}

// fmap [P][C] -> packed [C][Npad] (zeros beyond P): the correlation volume's B operand
__global__ __launch_bounds__(256) void flow_pack_kernel(int P, int C, int Npad, const float* __restrict__ fmap, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)C * Npad) return;
    const int c = (int)(i / Npad), n = (int)(i - (long long)c * Npad);
    out[i] = n < P ? fmap[(long long)n * C + c] : 0.0f;
}

__global__ __launch_bounds__(256) void flow_prep_kernel(int h, int w, int factor, int Hp, int Wp, int pad_top, int pad_left,
                                                         const unsigned char* __restrict__ img, float* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Hp * Wp) return;
    const int y = i / Wp, x = i - y * Wp;
    const int hs = h / factor, ws = w / factor;
    const int sy = min(max(y - pad_top, 0), hs - 1), sx = min(max(x - pad_left, 0), ws - 1);
    const int shift = factor == 1 ? 0 : factor == 2 ? 2 : 4;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        int s = 0;
        for (int dy = 0; dy < factor; dy++)
            for (int dx = 0; dx < factor; dx++) s += img[((long long)(sy * factor + dy) * w + (sx * factor + dx)) * 3 + c];
        if (shift) {   // round half to even
            const int half = 1 << (shift - 1);
            s = (s + half - 1 + ((s >> shift) & 1)) >> shift;
        }
        out[(long long)i * 3 + c] = 2.0f * ((float)s / 255.0f) - 1.0f;
    }
}

// ---- instance norm
__global__ __launch_bounds__(256) void flow_in_sums_kernel(int HW, int C, int R, int nchunks, const float* __restrict__ x,
                                                            double* __restrict__ partials)
{
    __shared__ double sh[256][2];
    const int t = threadIdx.x, c = t % C, r = t / C;
    const int chunk = blockIdx.x, n = blockIdx.y;
    const int p1 = min(HW, (chunk + 1) * IN_CHUNK);
    double s = 0.0, ss = 0.0;
    for (int p = chunk * IN_CHUNK + r; p < p1; p += R) {
        const double v = (double)x[((long long)n * HW + p) * C + c];
        s += v;
        ss += v * v;
    }
    sh[t][0] = s;
    sh[t][1] = ss;
    __syncthreads();
    if (r == 0) {
        for (int rr = 1; rr < R; rr++) {
            s += sh[rr * C + c][0];
            ss += sh[rr * C + c][1];
        }
        double* o = partials + ((long long)(n * C + c) * nchunks + chunk) * RED_STRIDE;
        o[0] = s;
        o[1] = ss;
    }
}

__global__ __launch_bounds__(RED_BLOCK) void flow_in_stats_kernel(int HW, int nchunks, const double* __restrict__ partials,
                                                                   float2* __restrict__ stats)
{
    double tot[2];
    tree_total<2>(nchunks, partials + (long long)blockIdx.x * nchunks * RED_STRIDE, tot);
    if (threadIdx.x == 0) {
        const double mean = tot[0] / (double)HW;
        double var = tot[1] / (double)HW - mean * mean;
        var = var > 0.0 ? var : 0.0;
        stats[blockIdx.x] = make_float2((float)mean, (float)(1.0 / sqrt(var + 1e-5)));
    }
}

__global__ __launch_bounds__(256) void flow_in_apply_kernel(long long n4, int HW, int C, const float4* __restrict__ x,
                                                             const float2* __restrict__ stats, int relu, const float4* __restrict__ res,
                                                             float4* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int c4 = C >> 2;
    const long long pix = i / c4;
    const int c = (int)(i - pix * c4) * 4, n = (int)(pix / HW);
    const float4 v = x[i];
    float y[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float2 st = stats[n * C + c + j];
        y[j] = (y[j] - st.x) * st.y;
        if (relu) y[j] = fmaxf(y[j], 0.0f);
    }
    if (res) {
        const float4 q = res[i];
        y[0] = fmaxf(q.x + y[0], 0.0f); y[1] = fmaxf(q.y + y[1], 0.0f);
        y[2] = fmaxf(q.z + y[2], 0.0f); y[3] = fmaxf(q.w + y[3], 0.0f);
    }
    out[i] = make_float4(y[0], y[1], y[2], y[3]);
}

// ---- correlation pyramid
__global__ __launch_bounds__(256) void flow_pool_kernel(long long n_out, int h, int w, const float* __restrict__ in, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_out) return;
    const int h2 = h >> 1, w2 = w >> 1;
    const long long row = i / (h2 * w2);
    const int rem = (int)(i - row * (h2 * w2));
    const int y = rem / w2, x = rem - y * w2;
    const float* p = in + row * ((long long)h * w) + (long long)(2 * y) * w + 2 * x;
    out[i] = (((p[0] + p[1]) + p[w]) + p[w + 1]) * 0.25f;
}

struct Pyramid { const float* lvl[FLOW_LEVELS]; int h[FLOW_LEVELS], w[FLOW_LEVELS]; };

__global__ __launch_bounds__(256) void flow_lookup_kernel(int h8, int w8, const float* __restrict__ flow, long long flow_stride,
                                                           int flow_off, const Pyramid py, float* __restrict__ out)
{
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long P = (long long)h8 * w8;
    if (i >= P * FLOW_CORR_CH) return;
    const long long p = i / FLOW_CORR_CH;
    const int ch = (int)(i - p * FLOW_CORR_CH);
    const int l = ch / (FLOW_WIN * FLOW_WIN), r = ch - l * (FLOW_WIN * FLOW_WIN);
    const int wi = r / FLOW_WIN, wj = r - wi * FLOW_WIN;
    const int py0 = (int)(p / w8), px0 = (int)(p - (long long)py0 * w8);
    const float* f = flow + p * flow_stride + flow_off;
    const float cx = (float)px0 + f[0], cy = (float)py0 + f[1];
    const float scale = 1.0f / (float)(1 << l);
    const float sx = cx * scale + (float)(wi - FLOW_RADIUS), sy = cy * scale + (float)(wj - FLOW_RADIUS);
    const int hl = py.h[l], wl = py.w[l];
    float v = 0.0f;
    if (sx > -1.0f && sx < (float)wl && sy > -1.0f && sy < (float)hl) {
        const float fx0 = floorf(sx), fy0 = floorf(sy);
        const int x0 = (int)fx0, y0 = (int)fy0;
        const float ax = sx - fx0, ay = sy - fy0, bx = (fx0 + 1.0f) - sx, by = (fy0 + 1.0f) - sy;
        const float* base = py.lvl[l] + p * ((long long)hl * wl);
        const bool xl = x0 >= 0, xr = x0 + 1 < wl, yt = y0 >= 0, yb = y0 + 1 < hl;
        const float nw = (xl && yt) ? base[(long long)y0 * wl + x0] : 0.0f;
        const float ne = (xr && yt) ? base[(long long)y0 * wl + x0 + 1] : 0.0f;
        const float sw = (xl && yb) ? base[(long long)(y0 + 1) * wl + x0] : 0.0f;
        const float se = (xr && yb) ? base[(long long)(y0 + 1) * wl + x0 + 1] : 0.0f;
        v = ((nw * (bx * by) + ne * (ax * by)) + sw * (bx * ay)) + se * (ax * ay);
    }
    out[i] = v;
}

// ---- GRU combine: mode 0: out = g h;  mode 1: out = (1 - g) h + g q
__global__ __launch_bounds__(256) void flow_gru_kernel(long long P, int C, int mode, const FlowSlice g, const FlowSlice h, const FlowSlice q,
                                                        const FlowSlice o)
{
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int c4 = C >> 2;
    if (i >= P * c4) return;
    const long long p = i / c4;
    const int c = (int)(i - p * c4) * 4;
    const float4 gv = *reinterpret_cast<const float4*>(g.base + p * g.stride + g.off + c);
    const float4 hv = *reinterpret_cast<const float4*>(h.base + p * h.stride + h.off + c);
    float4 r;
    if (mode == 0) {
        r = make_float4(gv.x * hv.x, gv.y * hv.y, gv.z * hv.z, gv.w * hv.w);
    } else {
        const float4 qv = *reinterpret_cast<const float4*>(q.base + p * q.stride + q.off + c);
        r = make_float4((1.0f - gv.x) * hv.x + gv.x * qv.x, (1.0f - gv.y) * hv.y + gv.y * qv.y, (1.0f - gv.z) * hv.z + gv.z * qv.z,
                        (1.0f - gv.w) * hv.w + gv.w * qv.w);
    }
    *reinterpret_cast<float4*>(const_cast<float*>(o.base) + p * o.stride + o.off + c) = r;
}

__global__ __launch_bounds__(256) void flow_upsample_kernel(int h8, int w8, const float* __restrict__ flow, long long flow_stride, int flow_off,
                                                             const float* __restrict__ mask, int pad_top, int pad_left, int h, int w,
                                                             float* __restrict__ out)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= h * w) return;
    const int Y = i / w, X = i - Y * w;
    const int Yp = Y + pad_top, Xp = X + pad_left;
    const int y = Yp >> 3, x = Xp >> 3, si = Yp & 7, sj = Xp & 7;
    const float* mk = mask + ((long long)y * w8 + x) * FLOW_MASK_CH + si * 8 + sj;
    float lg[9], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        lg[k] = 0.25f * mk[k * 64];
        mx = fmaxf(mx, lg[k]);
    }
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        lg[k] = expf(lg[k] - mx);
        sum += lg[k];
    }
    float ux = 0.0f, uy = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        if (yy < 0 || yy >= h8 || xx < 0 || xx >= w8) continue;
        const float* f = flow + ((long long)yy * w8 + xx) * flow_stride + flow_off;
        const float wk = lg[k] / sum;
        ux += wk * (8.0f * f[0]);
        uy += wk * (8.0f * f[1]);
    }
    out[(long long)i * 2] = ux;
    out[(long long)i * 2 + 1] = uy;
}

// ---- host helpers
inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
// columns of the packed weights: the matrix kernel's tiles, or the thin kernel's one float4 a row
inline int packed_n(int Cout) { return Cout <= FC_THIN ? FC_THIN : round_up(Cout, FC_BN); }
inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

const char* slice_error(const gsr_flow_slice& s, bool need16)
{
    if (!s.base) return "required pointer is null";
    if (s.channels < 1 || s.offset < 0 || s.stride < (long long)s.offset + s.channels) return "a slice does not fit its buffer";
    if (!aligned(s.base, 4)) return "a buffer must be 4-byte aligned";
    if (need16 && (!aligned(s.base, 16) || (s.channels & 3) || (s.offset & 3) || (s.stride & 3))) return "a slice must be 16-byte aligned";
    return nullptr;
}
inline FlowSlice slice_of(const gsr_flow_slice& s) { return FlowSlice{s.base, s.stride, s.offset, s.channels}; }

int launch_conv(const ConvArgs& a, bool vec, hipStream_t st)
{
    if (a.Cout <= FC_THIN) {
        const long long blocks = (a.M + 3) / 4;
        if (blocks > 0x7fffffffll) return fail_msg("gsr_flow_conv: too many output pixels");
        if (vec) flow_conv_thin_kernel<true><<<(unsigned)blocks, 256, 0, st>>>(a);
        else flow_conv_thin_kernel<false><<<(unsigned)blocks, 256, 0, st>>>(a);
        GSR_CHECK_LAUNCH("flow_conv_thin_kernel");
        return 0;
    }
    const long long mb = (a.M + FC_BM - 1) / FC_BM;
    if (mb > 0x7fffffffll) return fail_msg("gsr_flow_conv: too many output pixels");
    const dim3 grid((unsigned)mb, (unsigned)(a.Npad / FC_BN));
    if (vec) flow_conv_kernel<true><<<grid, FC_THREADS, 0, st>>>(a);
    else flow_conv_kernel<false><<<grid, FC_THREADS, 0, st>>>(a);
    GSR_CHECK_LAUNCH("flow_conv_kernel");
    return 0;
}

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

int gsr_flow_packed_k(int K) { return K > 0 ? round_up(K, FC_BK) : 0; }
int gsr_flow_packed_n(int Cout) { return Cout > 0 ? packed_n(Cout) : 0; }

int gsr_flow_prep_image(int h, int w, const unsigned char* image, int factor, float* out, gsr_stream_t stream)
{
    clear_error();
    if (factor != 1 && factor != 2 && factor != 4) return fail_msg("gsr_flow_prep_image: factor must be 1, 2 or 4");
    if (h < factor || w < factor || h % factor || w % factor) return fail_msg("gsr_flow_prep_image: the size must be a positive multiple of factor");
    if ((long long)h * w >= (1ll << 29)) return fail_msg("gsr_flow_prep_image: image too large");
    if (!image || !out) return fail_msg("gsr_flow_prep_image: required pointer is null");
    if (!aligned(out, 4)) return fail_msg("gsr_flow_prep_image: out must be 4-byte aligned");
    const int hs = h / factor, ws = w / factor;
    const int ph = (8 - hs % 8) % 8, pw = (8 - ws % 8) % 8;
    const int Hp = hs + ph, Wp = ws + pw;
    flow_prep_kernel<<<(Hp * Wp + 255) / 256, 256, 0, (hipStream_t)stream>>>(h, w, factor, Hp, Wp, ph / 2, pw / 2, image, out);
    GSR_CHECK_LAUNCH("flow_prep_kernel");
    return 0;
}

int gsr_flow_conv(const gsr_flow_conv_desc* d, gsr_stream_t stream)
{
    clear_error();
    if (!d) return fail_msg("gsr_flow_conv: required pointer is null");
    if (d->N < 1 || d->H < 1 || d->W < 1) return fail_msg("gsr_flow_conv: sizes must be positive");
    const int kh = d->KH, kw = d->KW;
    if (!((kh == 1 && kw == 1) || (kh == 3 && kw == 3) || (kh == 7 && kw == 7) || (kh == 1 && kw == 5) || (kh == 5 && kw == 1)))
        return fail_msg("gsr_flow_conv: the kernel must be 1x1, 3x3, 7x7, 1x5 or 5x1");
    if (d->stride != 1 && d->stride != 2) return fail_msg("gsr_flow_conv: stride must be 1 or 2");
    if (d->n_in < 1 || d->n_in > 3) return fail_msg("gsr_flow_conv: between 1 and 3 input slices");
    if (d->act < 0 || d->act > 3) return fail_msg("gsr_flow_conv: unknown activation");
    if (d->Cout < 2 || d->Cout > 576) return fail_msg("gsr_flow_conv: Cout must be between 2 and 576");
    ConvArgs a = {};
    bool vec = true;
    for (int i = 0; i < d->n_in; i++) {
        if (const char* e = slice_error(d->in[i], false)) return fail_msg((std::string("gsr_flow_conv: ") + e).c_str());
        vec = vec && !slice_error(d->in[i], true);
        a.in[i] = slice_of(d->in[i]);
        a.Cin += d->in[i].channels;
    }
    if (a.Cin < 2 || a.Cin > 384) return fail_msg("gsr_flow_conv: Cin must be between 2 and 384");
    if (d->out.channels != d->Cout) return fail_msg("gsr_flow_conv: the output slice must hold Cout channels");
    if (const char* e = slice_error(d->out, false)) return fail_msg((std::string("gsr_flow_conv: ") + e).c_str());
    if (d->residual.base) {
        if (d->residual.channels != d->Cout) return fail_msg("gsr_flow_conv: the residual slice must hold Cout channels");
        if (const char* e = slice_error(d->residual, false)) return fail_msg((std::string("gsr_flow_conv: ") + e).c_str());
    }
    if (!d->weights || !d->bias) return fail_msg("gsr_flow_conv: required pointer is null");
    if ((d->scale == nullptr) != (d->shift == nullptr)) return fail_msg("gsr_flow_conv: scale and shift come together");
    if (!aligned(d->weights, 16) || !aligned(d->bias, 4) || !aligned(d->scale, 4) || !aligned(d->shift, 4))
        return fail_msg("gsr_flow_conv: weights must be 16-byte aligned, bias, scale and shift 4-byte aligned");
    a.N = d->N; a.H = d->H; a.W = d->W; a.KH = kh; a.KW = kw; a.S = d->stride; a.PH = kh / 2; a.PW = kw / 2;
    a.Ho = (d->H + 2 * a.PH - kh) / a.S + 1;
    a.Wo = (d->W + 2 * a.PW - kw) / a.S + 1;
    a.M = (long long)d->N * a.Ho * a.Wo;
    if ((long long)d->N * d->H * d->W >= (1ll << 31) || a.M >= (1ll << 31)) return fail_msg("gsr_flow_conv: too many pixels");
    a.K = kh * kw * a.Cin; a.Cout = d->Cout; a.Npad = packed_n(d->Cout); a.n_in = d->n_in;
    a.w = d->weights; a.bias = d->bias; a.scale = d->scale; a.shift = d->shift; a.alpha = 1.0f; a.act = d->act;
    a.out = const_cast<float*>(d->out.base); a.out_stride = d->out.stride; a.out_off = d->out.offset;
    a.res = d->residual.base; a.res_stride = d->residual.stride; a.res_off = d->residual.offset; a.res_relu = d->residual_relu;
    return launch_conv(a, vec, (hipStream_t)stream);
}

int gsr_flow_pack_features(int P, int C, const float* fmap, float* packed, gsr_stream_t stream)
{
    clear_error();
    if (P < 1 || C < 1 || C % FC_BK) return fail_msg("gsr_flow_pack_features: P must be positive and C a positive multiple of 16");
    if (!fmap || !packed) return fail_msg("gsr_flow_pack_features: required pointer is null");
    if (!aligned(fmap, 4) || !aligned(packed, 16)) return fail_msg("gsr_flow_pack_features: packed must be 16-byte aligned");
    const int Npad = round_up(P, FC_BN);
    const long long n = (long long)C * Npad;
    flow_pack_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(P, C, Npad, fmap, packed);
    GSR_CHECK_LAUNCH("flow_pack_kernel");
    return 0;
}

int gsr_flow_corr_volume(int P1, int P2, int C, const float* fmap1, const float* packed2, float* volume, gsr_stream_t stream)
{
    clear_error();
    if (P1 < 1 || P2 < 1 || C < 4 || C % FC_BK) return fail_msg("gsr_flow_corr_volume: sizes must be positive and C a multiple of 16");
    if (!fmap1 || !packed2 || !volume) return fail_msg("gsr_flow_corr_volume: required pointer is null");
    if (!aligned(fmap1, 16) || !aligned(packed2, 16) || !aligned(volume, 4)) return fail_msg("gsr_flow_corr_volume: inputs must be 16-byte aligned");
    int e2 = 0;
    while ((1 << e2) < C) e2 += 2;          // alpha = 1 / sqrt(C) must be exact: C a power of four
    if ((1 << e2) != C) return fail_msg("gsr_flow_corr_volume: C must be a power of four");
    ConvArgs a = {};
    a.N = 1; a.H = 1; a.W = P1; a.Ho = 1; a.Wo = P1; a.KH = a.KW = 1; a.S = 1; a.M = P1;
    a.Cin = a.K = C; a.Cout = P2; a.Npad = round_up(P2, FC_BN); a.n_in = 1;
    a.in[0] = FlowSlice{fmap1, C, 0, C};
    a.in[1] = a.in[2] = FlowSlice{fmap1, C, 0, 0};
    a.w = packed2; a.alpha = 1.0f / (float)(1 << (e2 / 2));
    a.out = volume; a.out_stride = P2;
    return launch_conv(a, true, (hipStream_t)stream);
}

size_t gsr_flow_instance_norm_workspace_bytes(int N, int HW, int C)
{
    if (N < 1 || HW < 1 || C < 1) return 0;
    const size_t nchunks = ((size_t)HW + IN_CHUNK - 1) / IN_CHUNK;
    return align_up((size_t)N * C * nchunks * RED_STRIDE * sizeof(double)) + align_up((size_t)N * C * sizeof(float2)) + 256;
}

int gsr_flow_instance_norm(int N, int HW, int C, const float* x, int relu, const float* residual, float* out, void* workspace,
                           gsr_stream_t stream)
{
    clear_error();
    if (N < 1 || HW < 1) return fail_msg("gsr_flow_instance_norm: sizes must be positive");
    if (C < 4 || C > 256 || (C & 3)) return fail_msg("gsr_flow_instance_norm: C must be a multiple of 4 between 4 and 256");
    if ((long long)N * HW * C >= (1ll << 33) || (long long)N * C >= (1ll << 24)) return fail_msg("gsr_flow_instance_norm: too large");
    if (!x || !out || !workspace) return fail_msg("gsr_flow_instance_norm: required pointer is null");
    if (!aligned(x, 16) || !aligned(out, 16) || !aligned(residual, 16) || !aligned(workspace, 16))
        return fail_msg("gsr_flow_instance_norm: arrays must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nchunks = (HW + IN_CHUNK - 1) / IN_CHUNK, R = 256 / C;
    double* partials = static_cast<double*>(workspace);
    float2* stats = reinterpret_cast<float2*>(static_cast<char*>(workspace) + align_up((size_t)N * C * nchunks * RED_STRIDE * sizeof(double)));
    flow_in_sums_kernel<<<dim3(nchunks, N), C * R, 0, st>>>(HW, C, R, nchunks, x, partials);
    flow_in_stats_kernel<<<N * C, RED_BLOCK, 0, st>>>(HW, nchunks, partials, stats);
    const long long n4 = (long long)N * HW * C / 4;
    flow_in_apply_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, st>>>(n4, HW, C, reinterpret_cast<const float4*>(x), stats, relu,
                                                                      reinterpret_cast<const float4*>(residual), reinterpret_cast<float4*>(out));
    GSR_CHECK_LAUNCH("flow instance norm kernels");
    return 0;
}

int gsr_flow_corr_pool(long long rows, int h, int w, const float* in, float* out, gsr_stream_t stream)
{
    clear_error();
    if (rows < 1 || h < 2 || w < 2) return fail_msg("gsr_flow_corr_pool: rows must be positive and the level at least 2 x 2");
    if (!in || !out) return fail_msg("gsr_flow_corr_pool: required pointer is null");
    if (!aligned(in, 4) || !aligned(out, 4)) return fail_msg("gsr_flow_corr_pool: arrays must be 4-byte aligned");
    const long long n = rows * (h / 2) * (w / 2), blocks = (n + 255) / 256;
    if ((long long)h * w >= (1ll << 31) || blocks > 0x7fffffffll) return fail_msg("gsr_flow_corr_pool: too large");
    flow_pool_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(n, h, w, in, out);
    GSR_CHECK_LAUNCH("flow_pool_kernel");
    return 0;
}

int gsr_flow_corr_lookup(int h8, int w8, int h2, int w2, const gsr_flow_slice* flow, const float* level0, const float* level1,
                         const float* level2, const float* level3, float* out, gsr_stream_t stream)
{
    clear_error();
    if (h8 < 1 || w8 < 1 || h2 < 8 || w2 < 8) return fail_msg("gsr_flow_corr_lookup: the volume's levels must be at least 1 x 1");
    if (!flow || !level0 || !level1 || !level2 || !level3 || !out) return fail_msg("gsr_flow_corr_lookup: required pointer is null");
    if (flow->channels != 2) return fail_msg("gsr_flow_corr_lookup: the flow slice must hold 2 channels");
    if (const char* e = slice_error(*flow, false)) return fail_msg((std::string("gsr_flow_corr_lookup: ") + e).c_str());
    if (!aligned(level0, 4) || !aligned(level1, 4) || !aligned(level2, 4) || !aligned(level3, 4) || !aligned(out, 4))
        return fail_msg("gsr_flow_corr_lookup: arrays must be 4-byte aligned");
    Pyramid py;
    py.lvl[0] = level0; py.lvl[1] = level1; py.lvl[2] = level2; py.lvl[3] = level3;
    py.h[0] = h2; py.w[0] = w2;
    for (int l = 1; l < FLOW_LEVELS; l++) { py.h[l] = py.h[l - 1] / 2; py.w[l] = py.w[l - 1] / 2; }
    const long long n = (long long)h8 * w8 * FLOW_CORR_CH, blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffll || (long long)h2 * w2 >= (1ll << 31)) return fail_msg("gsr_flow_corr_lookup: too large");
    flow_lookup_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(h8, w8, flow->base, flow->stride, flow->offset, py, out);
    GSR_CHECK_LAUNCH("flow_lookup_kernel");
    return 0;
}

int gsr_flow_gru_combine(long long P, int mode, const gsr_flow_slice* gate, const gsr_flow_slice* h, const gsr_flow_slice* q,
                         const gsr_flow_slice* out, gsr_stream_t stream)
{
    clear_error();
    if (P < 1) return fail_msg("gsr_flow_gru_combine: P must be positive");
    if (mode != 0 && mode != 1) return fail_msg("gsr_flow_gru_combine: mode must be 0 (r h) or 1 ((1 - z) h + z q)");
    if (!gate || !h || !out || (mode == 1 && !q)) return fail_msg("gsr_flow_gru_combine: required pointer is null");
    const gsr_flow_slice* all[4] = {gate, h, out, mode == 1 ? q : gate};
    for (const gsr_flow_slice* s : all) {
        if (const char* e = slice_error(*s, true)) return fail_msg((std::string("gsr_flow_gru_combine: ") + e).c_str());
        if (s->channels != gate->channels) return fail_msg("gsr_flow_gru_combine: the slices must hold the same channels");
    }
    const long long n = P * (gate->channels / 4), blocks = (n + 255) / 256;
    if (blocks > 0x7fffffffll) return fail_msg("gsr_flow_gru_combine: too large");
    flow_gru_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(P, gate->channels, mode, slice_of(*gate), slice_of(*h),
                                                                      slice_of(*all[3]), slice_of(*out));
    GSR_CHECK_LAUNCH("flow_gru_kernel");
    return 0;
}

int gsr_flow_upsample(int h8, int w8, const gsr_flow_slice* flow, const float* mask, int pad_top, int pad_left, int h, int w, float* out,
                      gsr_stream_t stream)
{
    clear_error();
    if (h8 < 1 || w8 < 1 || h < 1 || w < 1) return fail_msg("gsr_flow_upsample: sizes must be positive");
    if (pad_top < 0 || pad_left < 0 || pad_top + (long long)h > 8ll * h8 || pad_left + (long long)w > 8ll * w8)
        return fail_msg("gsr_flow_upsample: the unpadded image must lie inside the padded one");
    if ((long long)h * w >= (1ll << 30)) return fail_msg("gsr_flow_upsample: too large");
    if (!flow || !mask || !out) return fail_msg("gsr_flow_upsample: required pointer is null");
    if (flow->channels != 2) return fail_msg("gsr_flow_upsample: the flow slice must hold 2 channels");
    if (const char* e = slice_error(*flow, false)) return fail_msg((std::string("gsr_flow_upsample: ") + e).c_str());
    if (!aligned(mask, 4) || !aligned(out, 4)) return fail_msg("gsr_flow_upsample: arrays must be 4-byte aligned");
    flow_upsample_kernel<<<(h * w + 255) / 256, 256, 0, (hipStream_t)stream>>>(h8, w8, flow->base, flow->stride, flow->offset, mask, pad_top,
                                                                             pad_left, h, w, out);
    GSR_CHECK_LAUNCH("flow_upsample_kernel");
    return 0;
}

}  // extern "C"
