// gsr_track.hip -- following points on the surface from frame to frame: tracking_face (gaustar_tools/tracking_util.py:34-148)
// and the binding step of find_face_of_tags (:20-27).  The reference does this on the host with trimesh, one Python loop per
// point and a full argmin over all face centres for every point an update displaced.  Here, over device tensors:
//   positions           track_positions_kernel     pos[k] = bary_to_point(verts[faces[id[k]]], bary[k])  (:70, every frame)
//   centres             track_centres_kernel       [F1,3] f64, one streaming pass per re-bind (:87)
//   rebind, survivors   track_survivors_kernel     a point whose face survived is re-expressed on that face (:94-107); the
//                                                  others are flagged for the to-do list; three integer counts
//   to-do list          track_todo_kernel          flag -> (torch.cumsum) -> scatter, its length in a device word
//   nearest centre      track_nn_kernel            the one O(K F1) step (:110-112): gsr_surface.h's tnn_search -- 256 threads, 16
//                                                  queries per workgroup, the centres staged through LDS in tiles of 1024
//                                                  (3 x 1024 doubles = 24 KiB) and split 16 ways among the lanes -- with f64
//                                                  queries, f64 centres and the rounded square root as the key
//   rebind, displaced   track_displaced_kernel     the nearest face's barycentrics, clamped and renormalised (:115-121)
// All arithmetic is float64 without contraction, every operation in the order include/gsr.h states.  No float atomics, no
// scratch: the counts are integer atomics, the search combines by the lexicographic (key, index) minimum.  The point type, the dot
// product, bary_to_point, point_to_bary (gsr_edit.hip's too), a face's vertices and that search are gsr_surface.h's, shared
// with gsr_eval.hip and gsr_stitch.hip.
//
// The square root.  numpy's argmin compares sqrt(d2), and two different d2 can share a rounded square root, so the minimum of
// (d2, index) is not the answer: the search takes the square root of every pair and keeps the (s, index) minimum.  The other
// way -- the smallest d2 first, then `hi`, the largest double whose square root rounds to sqrt(d2min), then a second pass for
// the lowest index with d2 <= hi -- was written, held to the same tests bit for bit, and measured against this one on an MI355X
// (tools/bench_tracking.py's case, profiles/tracking_config_c.txt).  On the update's own mask, 5 844 of 81 920 points searching
// 98 288 centres, the whole rebind took 1.15-1.21 ms with a square root per pair (two runs) and 1.23 ms in two passes: no
// difference beyond the spread between runs.  With all 81 920 points searching (8.05 x 10^9 pairs) 7.86-7.93 ms against
// 7.16 ms: the two passes are a tenth faster where the search is everything.  An update displaces a few per cent of the points,
// so the one-pass kernel, half the code, stayed; if whole-mesh searches become the common call, the other form is the one to
// bring back.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_surface.h"

#pragma clang fp contract(off)

namespace gsr {

namespace {

constexpr int TR_BLOCK = MESH_BLOCK;
constexpr int TNN_TILE = 1024;      // centres staged in LDS at once: 3 x 1024 doubles = 24 KiB

__device__ __forceinline__ void wave_count(bool mine, int* __restrict__ word)
{
    const unsigned long long m = __ballot(mine);
    if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(word, __popcll(m));
}

// pos [K,3]; a row whose id, face or vertices are not valid is NaN (and err says why)
__global__ void __launch_bounds__(TR_BLOCK) track_positions_kernel(int K, int F, int V, const int* __restrict__ faces,
                                                                   const double* __restrict__ verts, const int* __restrict__ ids,
                                                                   const double* __restrict__ bary, double* __restrict__ pos,
                                                                   int* __restrict__ err)
{
    const int k = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (k >= K) return;
    const double nan = __builtin_nan("");
    D3 out = {nan, nan, nan}, t0, t1, t2;
    const int id = ids[k];
    if ((unsigned)id >= (unsigned)F) atomicOr(err, MESH_ERR_INDEX);
    else if (face_verts(faces, verts, id, V, t0, t1, t2, err)) out = bary_to_point(t0, t1, t2, load3(bary, (size_t)k));
    store3(pos, (size_t)k, out);
}

// centres [F,3] = ((t0 + t1) + t2) / 3.0; NaN for a face left out
__global__ void __launch_bounds__(TR_BLOCK) track_centres_kernel(int F, int V, const int* __restrict__ faces,
                                                                 const double* __restrict__ verts, double* __restrict__ centres,
                                                                 int* __restrict__ err)
{
    const int f = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (f >= F) return;
    const double nan = __builtin_nan("");
    D3 out = {nan, nan, nan}, t0, t1, t2;
    if (face_verts(faces, verts, f, V, t0, t1, t2, err))
        out = {((t0.x + t1.x) + t2.x) / 3.0, ((t0.y + t1.y) + t2.y) / 3.0, ((t0.z + t1.z) + t2.z) / 3.0};
    store3(centres, (size_t)f, out);
}

// ids, bary: in place for the points that keep their face.  flag [K] int32 = 1 for a point that goes on the to-do list.
// stats [3] int32 (zero before): kept, moved off its face, lost.  A point the err word speaks of is in none of them.
__global__ void __launch_bounds__(TR_BLOCK) track_survivors_kernel(int K, int F0, int F1, int V1, const unsigned char* __restrict__ mask,
                                                                   const int* __restrict__ rank, const int* __restrict__ faces,
                                                                   const double* __restrict__ verts, const double* __restrict__ pos,
                                                                   int* __restrict__ ids, double* __restrict__ bary, int* __restrict__ flag,
                                                                   int* __restrict__ stats, int* __restrict__ err)
{
    const int k = blockIdx.x * TR_BLOCK + threadIdx.x;
    int state = 0;                                           // 1 kept, 2 moved, 3 lost
    if (k < K) {
        const int id = ids[k];
        const D3 p = load3(pos, (size_t)k);
        if ((unsigned)id >= (unsigned)F0) atomicOr(err, MESH_ERR_INDEX);
        else if (!finite3(p)) atomicOr(err, MESH_ERR_NAN);
        else if (!mask[id]) state = 3;
        else {
            const int j = rank[id];
            D3 t0, t1, t2;
            if ((unsigned)j >= (unsigned)F1) atomicOr(err, MESH_ERR_INDEX);
            else if (face_verts(faces, verts, j, V1, t0, t1, t2, err)) {
                const D3 nb = point_to_bary(t0, t1, t2, p);
                if (nb.x >= 0. && nb.y >= 0. && nb.z >= 0.) {   // (NaN fails, as in numpy)
                    ids[k] = j;
                    store3(bary, (size_t)k, nb);
                    state = 1;
                } else state = 2;
            }
        }
        flag[k] = state >= 2;
    }
    wave_count(state == 1, stats);
    wave_count(state == 2, stats + 1);
    wave_count(state == 3, stats + 2);
}

// scan: the INCLUSIVE scan of flag.  todo [n_todo] = the flagged k, ascending; *n_todo = their number.
__global__ void __launch_bounds__(TR_BLOCK) track_todo_kernel(int K, const int* __restrict__ flag, const int* __restrict__ scan,
                                                              int* __restrict__ todo, int* __restrict__ n_todo)
{
    const int k = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (k >= K) return;
    const int s = scan[k];
    if (flag[k] && s >= 1 && s <= K) todo[s - 1] = k;
    if (k == K - 1) *n_todo = s < 0 ? 0 : (s > K ? K : s);
}

// idx [slot] int32 = the lowest j among those with the smallest sqrt((dx dx + dy dy) + dz dz), d = query - centre_j; slot s <
// n = (n_live ? *n_live : K) is query (list ? list[s] : s).  grid = ceil(K / 16): the surplus workgroups exit on n.  A query or
// centre that is NaN ranks nothing; idx stays inside [0, F1) even then.
__global__ void __launch_bounds__(TNN_BLOCK) track_nn_kernel(int K, const int* __restrict__ list, const int* __restrict__ n_live, int F1,
                                                             const double* __restrict__ q, const double* __restrict__ c,
                                                             int* __restrict__ idx)
{
    int n = n_live ? *n_live : K;
    n = n < K ? n : K;
    if (blockIdx.x * TNN_QUERIES >= n) return;               // (the whole workgroup, ahead of tnn_search's barriers)
    const int slot = blockIdx.x * TNN_QUERIES + tnn_query();
    const bool live = slot < n;
    double qx = 0., qy = 0., qz = 0.;
    if (live) {
        int k = list ? list[slot] : slot;
        k = (unsigned)k < (unsigned)K ? k : 0;
        qx = q[3 * (size_t)k]; qy = q[3 * (size_t)k + 1]; qz = q[3 * (size_t)k + 2];
    }
    double bd;
    int bi;
    tnn_search<3, TNN_TILE, 4>(
        F1, bd, bi,
        [&](double (*tile)[TNN_TILE], int base, int m) {
            const double* src = c + 3 * (size_t)base;
            for (int e = threadIdx.x; e < 3 * m; e += TNN_BLOCK) tile[e % 3][e / 3] = src[e];
        },
        [&](const double (*tile)[TNN_TILE], int j) { return sqrt(tnn_d2(tile, j, qx, qy, qz)); });
    if (tnn_owner() && live) idx[slot] = bi == TNN_NONE ? 0 : bi;
}

// slot s < n (as in track_nn_kernel) is point k and takes face j = idx[s]: ids_out[k] = j, bary_out[k] = point_to_bary(face j,
// pos[k]); with `clamp`, if any component is < 0: nb = max(nb, 0), then nb / ((nb0 + nb1) + nb2), and a component that is
// still not >= 0 sets MESH_ERR_DEGENERATE (:118-125).
__global__ void __launch_bounds__(TR_BLOCK) track_displaced_kernel(int K, const int* __restrict__ list, const int* __restrict__ n_live,
                                                                   const int* __restrict__ idx, int F1, int V1, const int* __restrict__ faces,
                                                                   const double* __restrict__ verts, const double* __restrict__ pos,
                                                                   int* __restrict__ ids, double* __restrict__ bary, int clamp,
                                                                   int* __restrict__ err)
{
    const int s = blockIdx.x * TR_BLOCK + threadIdx.x;
    int n = n_live ? *n_live : K;
    n = n < K ? n : K;
    if (s >= n) return;
    const int k = list ? list[s] : s;
    if ((unsigned)k >= (unsigned)K) { atomicOr(err, MESH_ERR_INDEX); return; }
    const int j = idx[s];
    const D3 p = load3(pos, (size_t)k);
    const double nan = __builtin_nan("");
    D3 nb = {nan, nan, nan}, t0, t1, t2;
    if ((unsigned)j >= (unsigned)F1) atomicOr(err, MESH_ERR_INDEX);
    else if (!finite3(p)) atomicOr(err, MESH_ERR_NAN);
    else if (face_verts(faces, verts, j, V1, t0, t1, t2, err)) {
        nb = point_to_bary(t0, t1, t2, p);
        if (clamp) {
            if (nb.x < 0. || nb.y < 0. || nb.z < 0.) {
                nb = {nb.x < 0. ? 0. : nb.x, nb.y < 0. ? 0. : nb.y, nb.z < 0. ? 0. : nb.z};
                const double sum = (nb.x + nb.y) + nb.z;
                nb = {nb.x / sum, nb.y / sum, nb.z / sum};
            }
            if (!(nb.x >= 0. && nb.y >= 0. && nb.z >= 0.)) atomicOr(err, MESH_ERR_DEGENERATE);
        }
    }
    ids[k] = (unsigned)j < (unsigned)F1 ? j : 0;
    store3(bary, (size_t)k, nb);
}

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

int gsr_track_nn_tile(void) { return TNN_TILE; }
int gsr_track_nn_queries(void) { return TNN_QUERIES; }

int gsr_track_positions(int K, int F, int V, const int* faces, const double* verts, const int* ids, const double* bary, double* pos,
                        int* err, gsr_stream_t stream)
{
    clear_error();
    if (K < 0 || F < 0 || V < 0) return fail_msg("gsr_track_positions: negative size");
    if (K == 0) return 0;
    if (!ids || !bary || !pos || !err || (F > 0 && !faces) || (V > 0 && !verts))
        return fail_msg("gsr_track_positions: required pointer is null");
    track_positions_kernel<<<mesh_blocks(K), TR_BLOCK, 0, (hipStream_t)stream>>>(K, F, V, faces, verts, ids, bary, pos, err);
    GSR_CHECK_LAUNCH("track_positions_kernel");
    return 0;
}

int gsr_track_centres(int F, int V, const int* faces, const double* verts, double* centres, int* err, gsr_stream_t stream)
{
    clear_error();
    if (F < 0 || V < 0) return fail_msg("gsr_track_centres: negative size");
    if (F == 0) return 0;
    if (!faces || !centres || !err || (V > 0 && !verts)) return fail_msg("gsr_track_centres: required pointer is null");
    track_centres_kernel<<<mesh_blocks(F), TR_BLOCK, 0, (hipStream_t)stream>>>(F, V, faces, verts, centres, err);
    GSR_CHECK_LAUNCH("track_centres_kernel");
    return 0;
}

int gsr_track_rebind_survivors(int K, int F0, int F1, int V1, const unsigned char* mask, const int* rank, const int* new_faces,
                               const double* new_verts, const double* pos, int* ids, double* bary, int* flag, int* stats, int* err,
                               gsr_stream_t stream)
{
    clear_error();
    if (K < 0 || F0 < 0 || F1 < 0 || V1 < 0) return fail_msg("gsr_track_rebind_survivors: negative size");
    if (!stats) return fail_msg("gsr_track_rebind_survivors: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    GSR_CHECK(hipMemsetAsync(stats, 0, 3 * sizeof(int), st));
    if (K == 0) return 0;
    if (!pos || !ids || !bary || !flag || !err || (F0 > 0 && (!mask || !rank)) || (F1 > 0 && !new_faces) || (V1 > 0 && !new_verts))
        return fail_msg("gsr_track_rebind_survivors: required pointer is null");
    track_survivors_kernel<<<mesh_blocks(K), TR_BLOCK, 0, st>>>(K, F0, F1, V1, mask, rank, new_faces, new_verts, pos, ids, bary, flag,
                                                                 stats, err);
    GSR_CHECK_LAUNCH("track_survivors_kernel");
    return 0;
}

int gsr_track_todo(int K, const int* flag, const int* flag_scan, int* todo, int* n_todo, gsr_stream_t stream)
{
    clear_error();
    if (K < 0) return fail_msg("gsr_track_todo: negative size");
    if (!n_todo) return fail_msg("gsr_track_todo: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    GSR_CHECK(hipMemsetAsync(n_todo, 0, sizeof(int), st));
    if (K == 0) return 0;
    if (!flag || !flag_scan || !todo) return fail_msg("gsr_track_todo: required pointer is null");
    track_todo_kernel<<<mesh_blocks(K), TR_BLOCK, 0, st>>>(K, flag, flag_scan, todo, n_todo);
    GSR_CHECK_LAUNCH("track_todo_kernel");
    return 0;
}

int gsr_track_nearest(int K, const int* list, const int* n_live, int F1, const double* queries, const double* centres, int* idx,
                      gsr_stream_t stream)
{
    clear_error();
    if (K < 0 || F1 < 0) return fail_msg("gsr_track_nearest: negative size");
    if (K == 0) return 0;
    if (F1 == 0) return fail_msg("gsr_track_nearest: no centres");
    if (!queries || !centres || !idx) return fail_msg("gsr_track_nearest: required pointer is null");
    track_nn_kernel<<<(unsigned)((K + TNN_QUERIES - 1) / TNN_QUERIES), TNN_BLOCK, 0, (hipStream_t)stream>>>(K, list, n_live, F1, queries,
                                                                                                           centres, idx);
    GSR_CHECK_LAUNCH("track_nn_kernel");
    return 0;
}

int gsr_track_rebind_displaced(int K, const int* list, const int* n_live, const int* idx, int F1, int V1, const int* new_faces,
                               const double* new_verts, const double* pos, int* ids, double* bary, int clamp, int* err,
                               gsr_stream_t stream)
{
    clear_error();
    if (K < 0 || F1 < 0 || V1 < 0) return fail_msg("gsr_track_rebind_displaced: negative size");
    if (K == 0) return 0;
    if (!idx || !pos || !ids || !bary || !err || (F1 > 0 && !new_faces) || (V1 > 0 && !new_verts))
        return fail_msg("gsr_track_rebind_displaced: required pointer is null");
    track_displaced_kernel<<<mesh_blocks(K), TR_BLOCK, 0, (hipStream_t)stream>>>(K, list, n_live, idx, F1, V1, new_faces, new_verts, pos,
                                                                                ids, bary, clamp, err);
    GSR_CHECK_LAUNCH("track_displaced_kernel");
    return 0;
}

}  // extern "C"
