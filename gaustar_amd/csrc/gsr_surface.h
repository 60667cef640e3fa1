// gsr_surface.h -- what the kernels that work in float64 on a mesh (gsr_track.hip, gsr_eval.hip, gsr_remesh.hip, gsr_edit.hip and
// gsr_stitch.hip's search) share: a point of three doubles, the dot and cross products, bary_to_point and point_to_bary as
// include/gsr.h states them, a face's three f64 vertices with the err word's checks, and tnn_search, the tiled (key, index)-
// minimum search of stitch_nn_kernel, track_nn_kernel and eval_closest_kernel: 16 queries to a workgroup of 256, a tile split
// 16 ways.
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
constexpr int TNN_NONE = 0x7fffffff;   // the index of a search in which no candidate ranked (every key NaN)

struct D3 { double x, y, z; };

__device__ __forceinline__ D3 load3(const double* __restrict__ p, size_t i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ __forceinline__ void store3(double* __restrict__ p, size_t i, D3 v) { p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z; }
__device__ __forceinline__ D3 sub3(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
// each component two rounded products and one subtraction
__device__ __forceinline__ D3 cross3(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot3(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ bool finite1(double x) { return (x - x) == 0.; }
__device__ __forceinline__ bool finite3(D3 a) { return finite1(a.x) && finite1(a.y) && finite1(a.z); }

// trimesh's barycentric_to_points: per coordinate (b0 t0 + b1 t1) + b2 t2
__device__ __forceinline__ D3 bary_to_point(D3 t0, D3 t1, D3 t2, D3 b)
{
    return {(b.x * t0.x + b.y * t1.x) + b.z * t2.x, (b.x * t0.y + b.y * t1.y) + b.z * t2.y, (b.x * t0.z + b.y * t1.z) + b.z * t2.z};
}

// trimesh's points_to_barycentric, method "cramer", as include/gsr.h states it
__device__ __forceinline__ D3 point_to_bary(D3 t0, D3 t1, D3 t2, D3 p)
{
    const D3 e0 = sub3(t1, t0), e1 = sub3(t2, t0), w = sub3(p, t0);
    const double d00 = dot3(e0, e0), d01 = dot3(e0, e1), d02 = dot3(e0, w), d11 = dot3(e1, e1), d12 = dot3(e1, w);
    const double inv = 1.0 / (d00 * d11 - d01 * d01);
    const double b2 = (d00 * d12 - d01 * d02) * inv;
    const double b1 = (d11 * d02 - d01 * d12) * inv;
    return {(1.0 - b1) - b2, b1, b2};
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

// A thread's place in a search workgroup: thread t = 64 wave + lane holds query (lane & 15) and slice 4 wave + (lane >> 4) of
// every tile.  Threads 0 .. 15 (slice 0 of each query) do what is done once per query: its checks, and after tnn_search its tail.
__device__ __forceinline__ int tnn_query() { return threadIdx.x & (TNN_QUERIES - 1); }
__device__ __forceinline__ bool tnn_owner() { return threadIdx.x < TNN_QUERIES; }

// (bd, bi) = the smallest key(tile, j) over candidates j in [0, M) and the LOWEST j that has it, (+inf, TNN_NONE) if no key is
// below +inf; valid in lanes < 16 of EVERY wave (tnn_combine).  The candidates pass through an LDS tile of ROWS x TILE doubles:
// stage(tile, base, n) writes candidates [base, base + n) to columns [0, n), all TNN_BLOCK threads taking part, between the two
// barriers here; key(tile, j) is this thread's query against column j.  The whole workgroup calls this, or none of it.
// UNROLL is the slice loop's unroll count (1: none).
template <int ROWS, int TILE, int UNROLL, class Stage, class Key>
__device__ __forceinline__ void tnn_search(int M, double& bd, int& bi, Stage stage, Key key)
{
    __shared__ double tile[ROWS][TILE];
    __shared__ double part_d[TNN_BLOCK / 64][TNN_QUERIES];
    __shared__ int part_i[TNN_BLOCK / 64][TNN_QUERIES];
    const int slice = (threadIdx.x >> 6) * 4 + ((threadIdx.x & 63) >> 4);
    double d_min = __builtin_inf();                          // (locals: with the loop on the references track_nn_kernel carried
    int j_min = TNN_NONE;                                    //  a second copy of the minimum, two VGPRs and two selects a pair)
    for (int base = 0; base < M; base += TILE) {
        const int n = M - base < TILE ? M - base : TILE;
        __syncthreads();                                     // (the tile before is read to its end)
        stage(tile, base, n);
        __syncthreads();
#pragma unroll UNROLL
        for (int j = slice; j < n; j += TNN_SLICES) {        // ascending index: `<` keeps the lowest among equals
            const double d = key(tile, j);
            if (d < d_min) { d_min = d; j_min = base + j; }
        }
    }
    tnn_combine(d_min, j_min, part_d, part_i);
    bd = d_min;
    bi = j_min;
}

// the squared distance from (qx, qy, qz) to column j of a tile of three rows x, y, z
template <int TILE>
__device__ __forceinline__ double tnn_d2(const double (*tile)[TILE], int j, double qx, double qy, double qz)
{
    const double dx = qx - tile[0][j], dy = qy - tile[1][j], dz = qz - tile[2][j];
    return (dx * dx + dy * dy) + dz * dz;
}

}  // namespace

}  // namespace gsr
