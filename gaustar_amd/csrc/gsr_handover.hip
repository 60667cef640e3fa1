// gsr_handover.hip -- the colours a frame hands to the next one: the colour mesh of get_color_mesh
// (gaustar_scene/sugar_model.py:578-588), the face colours update_mesh_topo carries through connect_two_meshes
// (gaustar_trainers/refined_mesh.py:183), and the SH dc a model starts with when it is built from a coloured mesh
// (sugar_model.py:235-240, :386).  Five plain memory-bound passes, one thread per output element; a colour is four bytes
// (r, g, b, a) written as one 32-bit word.
//
//   face colours    handover_face_color_kernel<G>   RGBA8 of a face from the SH dc of its G Gaussians: numpy's result for
//                                                   np.clip(np.int32(SH2RGB(np.average(dc, axis=1)) * 255), 0, 255) on f32
//   vertex -> face  handover_vertex_to_face_kernel  trimesh's vertex -> face colour conversion as this project states it: a vertex
//                                                   colour in [0,1] becomes clip(rint(255 c), 0, 255), a face the floor of the
//                                                   integer mean of its three vertices
//   face -> vertex  handover_scatter_kernel         trimesh's face -> vertex conversion as this project states it: per vertex the
//                   handover_vertex_mean_kernel     floor of the integer mean of its incident faces whose alpha is not 0; 32-bit
//                                                   integer adds, so the sum does not depend on their order
//   SH dc           handover_sh_dc_kernel           RGB2SH of the barycentric blend of a face's three vertex colours
//   gather          handover_gather_kernel          the face colours of an updated mesh from every face's origin
// Filled faces carry (0, 0, 0, 0) and are left out of the vertex means: trimesh's fill_holes would give them a default colour.
// Every value a kernel here reads was written by an earlier launch, except the integer adds of the scatter.  No float atomics,
// no scratch, no LDS.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_internal.h"
#include "gsr_mesh.h"

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int HO_BLOCK = MESH_BLOCK;
constexpr int HO_FILLED = -2147483647 - 1; // a face_origin entry: made by fill_small_holes
constexpr float HO_C0 = 0.28209479177387814f;

__device__ __forceinline__ unsigned pack_rgba(int r, int g, int b, int a)
{
    return (unsigned)r | ((unsigned)g << 8) | ((unsigned)b << 16) | ((unsigned)a << 24);
}

// np.clip(np.int32(x), 0, 255) for every x whose truncation fits an int32; beyond that (and for NaN) numpy's cast is not
// defined, and this saturates (NaN: 0).
__device__ __forceinline__ int trunc_clip(float x)
{
    return x >= 255.f ? 255 : (x > 0.f ? (int)x : 0);
}

// clip(rint(255 c), 0, 255), ties to even; NaN: 0
__device__ __forceinline__ int unit_to_u8(float c)
{
    const float r = rintf(c * 255.f);
    return r >= 255.f ? 255 : (r > 0.f ? (int)r : 0);
}

// ---------------------------------------------------------------------------------------------------- face colours
// sh_dc [F G,3], face-major.  m = (((x0 + x1) + ...) + x_{G-1}) / G, c = (m C0 + 0.5) 255, every operation rounded to f32.
template <int G>
__global__ void __launch_bounds__(HO_BLOCK) handover_face_color_kernel(int F, const float* __restrict__ sh_dc, unsigned* __restrict__ rgba)
{
    const int f = blockIdx.x * HO_BLOCK + threadIdx.x;
    if (f >= F) return;
    const float* x = sh_dc + 3 * (size_t)G * f;
    int out[3];
    for (int c = 0; c < 3; ++c) {
        float s = x[c];
        for (int g = 1; g < G; ++g) s = s + x[3 * g + c];
        const float m = s / (float)G;
        const float v = (m * HO_C0 + 0.5f) * 255.f;
        out[c] = trunc_clip(v);
    }
    rgba[f] = pack_rgba(out[0], out[1], out[2], 255);
}

// ---------------------------------------------------------------------------------------------------- vertex -> face
// colors [V][stride] f32, the first three of a row are r, g, b
__device__ __forceinline__ unsigned face_of_vertex_colors(const float* __restrict__ colors, int stride, const int (&v)[3])
{
    int out[3];
    for (int c = 0; c < 3; ++c) {
        const int u0 = unit_to_u8(colors[(size_t)stride * v[0] + c]);
        const int u1 = unit_to_u8(colors[(size_t)stride * v[1] + c]);
        const int u2 = unit_to_u8(colors[(size_t)stride * v[2] + c]);
        out[c] = (u0 + u1 + u2) / 3;
    }
    return pack_rgba(out[0], out[1], out[2], 255);
}

__global__ void __launch_bounds__(HO_BLOCK) handover_vertex_to_face_kernel(int F, int V, const int* __restrict__ faces,
                                                                           const float* __restrict__ colors, int stride,
                                                                           unsigned* __restrict__ rgba, int* __restrict__ err)
{
    const int f = blockIdx.x * HO_BLOCK + threadIdx.x;
    if (f >= F) return;
    int v[3];
    if (!mesh_face(faces, f, V, v)) {
        atomicOr(err, MESH_ERR_INDEX);
        rgba[f] = 0u;
        return;
    }
    rgba[f] = face_of_vertex_colors(colors, stride, v);
}

// ---------------------------------------------------------------------------------------------------- face -> vertex
// sums [V][4] int32 (zero before): the r, g, b sums and the number of the incident faces with alpha != 0.  A face that names a
// vertex twice counts twice there, as a row of the face-vertex incidence matrix would.
__global__ void __launch_bounds__(HO_BLOCK) handover_scatter_kernel(int F, int V, const int* __restrict__ faces,
                                                                    const unsigned* __restrict__ face_rgba, int* __restrict__ sums,
                                                                    int* __restrict__ err)
{
    const int f = blockIdx.x * HO_BLOCK + threadIdx.x;
    if (f >= F) return;
    int v[3];
    if (!mesh_face(faces, f, V, v)) {
        atomicOr(err, MESH_ERR_INDEX);
        return;
    }
    const unsigned c = face_rgba[f];
    if ((c >> 24) == 0u) return;
    for (int k = 0; k < 3; ++k) {
        int* s = sums + 4 * (size_t)v[k];
        atomicAdd(s + 0, (int)(c & 0xffu));
        atomicAdd(s + 1, (int)((c >> 8) & 0xffu));
        atomicAdd(s + 2, (int)((c >> 16) & 0xffu));
        atomicAdd(s + 3, 1);
    }
}

__global__ void __launch_bounds__(HO_BLOCK) handover_vertex_mean_kernel(int V, const int4* __restrict__ sums, unsigned* __restrict__ vert_rgba)
{
    const int v = blockIdx.x * HO_BLOCK + threadIdx.x;
    if (v >= V) return;
    const int4 s = sums[v];
    vert_rgba[v] = s.w > 0 ? pack_rgba(s.x / s.w, s.y / s.w, s.z / s.w, 255) : 0u;
}

// ---------------------------------------------------------------------------------------------------- SH dc
// One thread per Gaussian g of face f.  c = (b_g0 v0 + b_g1 v1) + b_g2 v2, dc = (c - 0.5) / C0: three rounded products, two
// rounded sums, a true division.  bary [G][3] f32 (harness.BARY_COORDS rounded to f32).
__global__ void __launch_bounds__(HO_BLOCK) handover_sh_dc_kernel(int F, int G, int V, const int* __restrict__ faces,
                                                                  const float* __restrict__ colors, int stride,
                                                                  const float* __restrict__ bary, float* __restrict__ sh_dc,
                                                                  int* __restrict__ err)
{
    const long long n = (long long)blockIdx.x * HO_BLOCK + threadIdx.x;
    if (n >= (long long)F * G) return;
    const int f = (int)(n / G), g = (int)(n - (long long)f * G);
    int v[3];
    float* o = sh_dc + 3 * (size_t)n;
    if (!mesh_face(faces, f, V, v)) {
        atomicOr(err, MESH_ERR_INDEX);
        o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
        return;
    }
    const float b0 = bary[3 * g], b1 = bary[3 * g + 1], b2 = bary[3 * g + 2];
    for (int c = 0; c < 3; ++c) {
        const float p0 = b0 * colors[(size_t)stride * v[0] + c];
        const float p1 = b1 * colors[(size_t)stride * v[1] + c];
        const float p2 = b2 * colors[(size_t)stride * v[2] + c];
        const float col = (p0 + p1) + p2;
        o[c] = (col - 0.5f) / HO_C0;
    }
}

// ---------------------------------------------------------------------------------------------------- gather
// origin [n]: k >= 0 = face k of the base colours, -1 - k = face k of the fusion mesh (coloured from its vertices as the
// vertex -> face kernel does), INT32_MIN = a filled face: (0, 0, 0, 0).
__global__ void __launch_bounds__(HO_BLOCK) handover_gather_kernel(int n, const int* __restrict__ origin, int Fb,
                                                                   const unsigned* __restrict__ base_rgba, int Ff, int Vf,
                                                                   const int* __restrict__ fusion_faces, const float* __restrict__ fusion_colors,
                                                                   int stride, unsigned* __restrict__ rgba, int* __restrict__ err)
{
    const int i = blockIdx.x * HO_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int o = origin[i];
    unsigned c = 0u;
    if (o >= 0) {
        if (o < Fb) c = base_rgba[o];
        else atomicOr(err, MESH_ERR_INDEX);
    } else if (o != HO_FILLED) {
        const int k = -1 - o;
        int v[3];
        if (k < Ff && mesh_face(fusion_faces, k, Vf, v)) c = face_of_vertex_colors(fusion_colors, stride, v);
        else atomicOr(err, MESH_ERR_INDEX);
    }
    rgba[i] = c;
}

bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

int gsr_handover_face_colors(int F, int G, const float* sh_dc, unsigned char* rgba, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F)) return fail_msg("gsr_handover_face_colors: negative size or too many faces");
    if (G != 1 && G != 3 && G != 4 && G != 6) return fail_msg("gsr_handover_face_colors: G must be 1, 3, 4 or 6");
    if (F == 0) return 0;
    if (!sh_dc || !rgba) return fail_msg("gsr_handover_face_colors: required pointer is null");
    if (misaligned4(rgba)) return fail_msg("gsr_handover_face_colors: rgba must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned* out = reinterpret_cast<unsigned*>(rgba);
    switch (G) {
    case 1: handover_face_color_kernel<1><<<mesh_blocks(F), HO_BLOCK, 0, st>>>(F, sh_dc, out); break;
    case 3: handover_face_color_kernel<3><<<mesh_blocks(F), HO_BLOCK, 0, st>>>(F, sh_dc, out); break;
    case 4: handover_face_color_kernel<4><<<mesh_blocks(F), HO_BLOCK, 0, st>>>(F, sh_dc, out); break;
    default: handover_face_color_kernel<6><<<mesh_blocks(F), HO_BLOCK, 0, st>>>(F, sh_dc, out); break;
    }
    GSR_CHECK_LAUNCH("handover_face_color_kernel");
    return 0;
}

int gsr_handover_vertex_to_face(int F, int V, const int* faces, const float* colors, int stride, unsigned char* rgba, int* err,
                                gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || V < 0) return fail_msg("gsr_handover_vertex_to_face: negative size or too many faces");
    if (stride < 3) return fail_msg("gsr_handover_vertex_to_face: a colour row holds at least r, g, b");
    if (F == 0) return 0;
    if (!faces || !rgba || !err || (V > 0 && !colors)) return fail_msg("gsr_handover_vertex_to_face: required pointer is null");
    if (misaligned4(rgba)) return fail_msg("gsr_handover_vertex_to_face: rgba must be 4-byte aligned");
    handover_vertex_to_face_kernel<<<mesh_blocks(F), HO_BLOCK, 0, (hipStream_t)stream>>>(F, V, faces, colors, stride,
                                                                                     reinterpret_cast<unsigned*>(rgba), err);
    GSR_CHECK_LAUNCH("handover_vertex_to_face_kernel");
    return 0;
}

int gsr_handover_face_to_vertex(int F, int V, const int* faces, const unsigned char* face_rgba, int* sums, unsigned char* vert_rgba,
                                int* err, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || V < 0 || V > 0x7fffffff / 4) return fail_msg("gsr_handover_face_to_vertex: negative size or too large a mesh");
    if (V == 0) return 0;
    if (!sums || !vert_rgba || (F > 0 && (!faces || !face_rgba || !err))) return fail_msg("gsr_handover_face_to_vertex: required pointer is null");
    if (misaligned4(vert_rgba) || (F > 0 && misaligned4(face_rgba))) return fail_msg("gsr_handover_face_to_vertex: colours must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(sums) & 15) return fail_msg("gsr_handover_face_to_vertex: sums must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    GSR_CHECK(hipMemsetAsync(sums, 0, 4 * sizeof(int) * (size_t)V, st));
    if (F > 0) handover_scatter_kernel<<<mesh_blocks(F), HO_BLOCK, 0, st>>>(F, V, faces, reinterpret_cast<const unsigned*>(face_rgba), sums, err);
    handover_vertex_mean_kernel<<<mesh_blocks(V), HO_BLOCK, 0, st>>>(V, reinterpret_cast<const int4*>(sums), reinterpret_cast<unsigned*>(vert_rgba));
    GSR_CHECK_LAUNCH("handover face-to-vertex kernels");
    return 0;
}

int gsr_handover_sh_dc(int F, int G, int V, const int* faces, const float* colors, int stride, const float* bary, float* sh_dc, int* err,
                       gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || V < 0) return fail_msg("gsr_handover_sh_dc: negative size or too many faces");
    if (G != 1 && G != 3 && G != 4 && G != 6) return fail_msg("gsr_handover_sh_dc: G must be 1, 3, 4 or 6");
    if (stride < 3) return fail_msg("gsr_handover_sh_dc: a colour row holds at least r, g, b");
    if (F == 0) return 0;
    if (!faces || !bary || !sh_dc || !err || (V > 0 && !colors)) return fail_msg("gsr_handover_sh_dc: required pointer is null");
    handover_sh_dc_kernel<<<mesh_blocks((long long)F * G), HO_BLOCK, 0, (hipStream_t)stream>>>(F, G, V, faces, colors, stride, bary, sh_dc, err);
    GSR_CHECK_LAUNCH("handover_sh_dc_kernel");
    return 0;
}

int gsr_handover_gather(int n, const int* origin, int Fb, const unsigned char* base_rgba, int Ff, int Vf, const int* fusion_faces,
                        const float* fusion_colors, int stride, unsigned char* rgba, int* err, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(n) || !mesh_faces_ok(Ff) || Fb < 0 || Vf < 0) return fail_msg("gsr_handover_gather: negative size or too many faces");
    if (stride < 3) return fail_msg("gsr_handover_gather: a colour row holds at least r, g, b");
    if (n == 0) return 0;
    if (!origin || !rgba || !err || (Fb > 0 && !base_rgba) || (Ff > 0 && (!fusion_faces || (Vf > 0 && !fusion_colors))))
        return fail_msg("gsr_handover_gather: required pointer is null");
    if (misaligned4(rgba) || (Fb > 0 && misaligned4(base_rgba))) return fail_msg("gsr_handover_gather: colours must be 4-byte aligned");
    handover_gather_kernel<<<mesh_blocks(n), HO_BLOCK, 0, (hipStream_t)stream>>>(n, origin, Fb, reinterpret_cast<const unsigned*>(base_rgba), Ff, Vf,
                                                                             fusion_faces, fusion_colors, stride,
                                                                             reinterpret_cast<unsigned*>(rgba), err);
    GSR_CHECK_LAUNCH("handover_gather_kernel");
    return 0;
}

}  // extern "C"
