// gsr_mesh.h -- what the mesh-surgery kernels (gsr_regions.hip, gsr_stitch.hip, gsr_splice.hip, gsr_handover.hip, gsr_track.hip,
// gsr_eval.hip, gsr_remesh.hip) share.
// Every call of those files that takes `int* err` ORs into one word, which gaustar_amd.regions may pass through calls of
// several files before its one decoder (gaustar_amd/_meshargs.py: raise_if) reads it: the bits are defined here and there.
#pragma once

namespace gsr {

constexpr int MESH_ERR_INDEX = 1;   // an index outside its array: a face's vertex, a list entry, a face_origin entry
constexpr int MESH_ERR_NAN = 2;     // a coordinate that is NaN (a region's box) or not finite (a nearest-vertex search)
constexpr int MESH_ERR_DUP = 4;     // a boundary list names a vertex twice
constexpr int MESH_ERR_DEGENERATE = 8;   // gsr_track.hip: a re-bound barycentric that is not >= 0 (a degenerate nearest face);
                                         // gsr_eval.hip: sampling weights that are not usable (no face with a positive, finite area)
constexpr int MESH_BLOCK = 256;     // the workgroup of every one-thread-per-element kernel of these files

inline unsigned mesh_blocks(long long n) { return (unsigned)((n + MESH_BLOCK - 1) / MESH_BLOCK); }

// 3 F face-edges are counted in an int
inline bool mesh_faces_ok(int F) { return F >= 0 && F <= 0x7fffffff / 3; }

// v = the three vertex indices of face f; true iff all of them lie in [0, V).  Nothing is indexed with them here.
__device__ __forceinline__ bool mesh_face(const int* __restrict__ faces, int f, int V, int (&v)[3])
{
    for (int k = 0; k < 3; ++k) v[k] = faces[3 * (size_t)f + k];
    return (unsigned)v[0] < (unsigned)V && (unsigned)v[1] < (unsigned)V && (unsigned)v[2] < (unsigned)V;
}

// the key of the undirected edge (a, b): min << 32 | max
__device__ __forceinline__ long long edge_key(int a, int b)
{
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return ((long long)lo << 32) | (long long)(unsigned)hi;
}

}  // namespace gsr
