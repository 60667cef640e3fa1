// gsr_v3.h -- the f32 vector of the fused mesh losses (gsr_mesh_reg.hip, gsr_mesh_lap.hip).  These run at the build's default
// contraction, the f32 composition they restate being no bit-for-bit target: the header sets no fp-contract pragma and is
// included ahead of any in the including file.  (gsr_producers.hip's V3, written with operators, is another type.)
#pragma once

namespace gsr {

namespace {

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 ld3(const float* __restrict__ v, int i) { return V3{v[3 * i], v[3 * i + 1], v[3 * i + 2]}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 mul(float s, V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 neg(V3 a) { return V3{-a.x, -a.y, -a.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

}  // namespace

}  // namespace gsr
