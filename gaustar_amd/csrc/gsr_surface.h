// gsr_surface.h -- what the kernels that work with points ON a mesh's surface (gsr_track.hip, gsr_eval.hip) share: a point of
// three doubles, the dot product and bary_to_point as include/gsr.h states them, a face's three f64 vertices with the err word's
// checks, and the (key, index) minimum of the searches that give 16 queries to a workgroup of 256 and split a tile 16 ways.
// All of it float64 without contraction: the pragma below stands in front of these functions (an including file's own pragma
// comes after its includes and would leave them contracted) and holds for the rest of the translation unit.
#pragma once
#include "gsr_mesh.h"

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int TNN_BLOCK = 256;      // four waves
constexpr int TNN_QUERIES = 16;     // queries of a workgroup: lane & 15 of every wave
constexpr int TNN_SLICES = 16;      // shares of a tile: 4 waves x (lane >> 4); slice s takes j = s, s + 16, ...

struct D3 { double x, y, z; };

__device__ __forceinline__ D3 load3(const double* __restrict__ p, size_t i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ void store3(double* __restrict__ p, size_t i, D3 v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }
__device__ __forceinline__ D3 sub3(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot3(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ bool finite1(double x) { return (x - x) == 0.; }
__device__ __forceinline__ bool finite3(D3 a) { return finite1(a.x) && finite1(a.y) && finite1(a.z); }

// trimesh's barycentric_to_points: per coordinate (b0 t0 + b1 t1) + b2 t2
__device__ __forceinline__ D3 bary_to_point(D3 t0, D3 t1, D3 t2, D3 b)
{
    return {(b.x * t0.x + b.y * t1.x) + b.z * t2.x, (b.x * t0.y + b.y * t1.y) + b.z * t2.y, (b.x * t0.z + b.y * t1.z) + b.z * t2.z};
}

// the three vertices of face f of a mesh of V vertices; false (and err) when an index is outside or a coordinate not finite
__device__ __forceinline__ bool face_verts(const int* __restrict__ faces, const double* __restrict__ verts, int f, int V,
                                           D3& t0, D3& t1, D3& t2, int* __restrict__ err)
{
    int v[3];
    if (!mesh_face(faces, f, V, v)) { atomicOr(err, MESH_ERR_INDEX); return false; }
    t0 = load3(verts, (size_t)v[0]); t1 = load3(verts, (size_t)v[1]); t2 = load3(verts, (size_t)v[2]);
    if (!(finite3(t0) && finite3(t1) && finite3(t2))) { atomicOr(err, MESH_ERR_NAN); return false; }
    return true;
}

// the lexicographic (key, index) minimum: the same whatever the order the parts are combined in
__device__ __forceinline__ void tnn_take(double& bd, int& bi, double od, int oi)
{
    if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
}

// the (key, index) minimum of a query's 16 slices -> lanes < 16 of every wave (lane = the query)
__device__ __forceinline__ void tnn_combine(double& bd, int& bi, double (*part_d)[TNN_QUERIES], int (*part_i)[TNN_QUERIES])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 16; m < 64; m <<= 1) {                      // the four slices of this wave
        const double od = __shfl_xor(bd, m);
        const int oi = __shfl_xor(bi, m);
        tnn_take(bd, bi, od, oi);
    }
    if (lane < TNN_QUERIES) { part_d[wave][lane] = bd; part_i[wave][lane] = bi; }
    __syncthreads();
    if (lane < TNN_QUERIES)
        for (int w = 0; w < TNN_BLOCK / 64; ++w) tnn_take(bd, bi, part_d[w][lane], part_i[w][lane]);
}

}  // namespace

}  // namespace gsr
