// gsr_regions.hip -- the front half of update_mesh_topo (gaustar_trainers/refined_mesh.py:463-693): which faces of the base mesh
// are re-meshed, the boxes around them, and the cuts of the base mesh and of the fused surface by those boxes.
//
// The reference does this on the host with trimesh (group_rows over the sorted edges, scipy's connected_components, update_faces,
// remove_unreferenced_vertices).  Here, over device tensors:
//   edge multiplicity   regions_edge_key_kernel    a 64-bit key (min << 32 | max) per face-edge, a sentinel outside the mask
//                       (torch.sort of the keys, as topology.py sorts its voxel keys)
//                       regions_edge_run_kernel    per sorted key the length of its run, written back to its face-edge; a run of
//                                                  exactly two face-edges of two different faces is an adjacency pair
//   components          uf_init / uf_hook / uf_flatten_kernel (gsr_unionfind.h)   union-find over the pairs: the larger root is pointed at the
//                                                  smaller by compare-and-swap, so a tree's root is its smallest face whatever
//                                                  order the hooks landed in; flatten finds it without a store to any other
//                                                  face's word and writes it to parent[f], once
//                       (torch.cumsum over the root flags)
//                       regions_label_kernel       dense labels in ascending order of the smallest face, faces per label
//   selection           regions_select_kernel      components above the face threshold, in label order
//                       regions_box_kernel         per kept component min / max over its faces' vertices and Gaussian centres
//   cut                 regions_inside_kernel, regions_cut_mark_kernel, (two cumsums), regions_cut_faces_kernel,
//                       regions_cut_verts_kernel, regions_gather_kernel
//   primitives          regions_boundary_kernel (find_boundary_verts, :84-111), regions_label_mask_kernel (get_outlier_cc_mask, :291-307)
// Every output is an integer or an exactly defined float: counts are integer adds, boxes integer min / max on an order-preserving
// encoding of the f32, ids come from scans.  No float atomics.
//
// Workgroups on different XCDs hook concurrently: every read of `parent` inside a find is an agent-scope atomic load, every
// write an agent-scope atomic store or compare-and-swap.
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_internal.h"
#include "gsr_mesh.h"
#include "gsr_unionfind.h"

namespace gsr {

namespace {

constexpr int RG_BLOCK = MESH_BLOCK;
constexpr long long RG_SENTINEL = 0x7fffffffffffffffll;   // above every key: min, max <= 2^31 - 1
constexpr int RG_WALK = 8;                                 // neighbours looked at before a run's end is found by bisection

struct RegionBox { double lo[3], hi[3]; };

// ---------------------------------------------------------------------------------------------------- edge multiplicity
// Face-edge e of face (a, b, c) is (a, b), (b, c), (c, a) for e = 0, 1, 2 (trimesh's faces_to_edges).
__global__ void __launch_bounds__(RG_BLOCK) regions_edge_key_kernel(int F, const int* __restrict__ faces, const unsigned char* __restrict__ mask,
                                                                    const unsigned char* __restrict__ colour, int cut,
                                                                    unsigned char* __restrict__ sel, long long* __restrict__ keys,
                                                                    int* __restrict__ err)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
    bool on = (!mask || mask[f]) && (!colour || (int)colour[f] >= cut);
    if ((a | b | c) < 0) { atomicOr(err, MESH_ERR_INDEX); on = false; }
    sel[f] = on;
    long long* k = keys + 3 * (size_t)f;
    k[0] = on ? edge_key(a, b) : RG_SENTINEL;
    k[1] = on ? edge_key(b, c) : RG_SENTINEL;
    k[2] = on ? edge_key(c, a) : RG_SENTINEL;
}

// n = 3 F sorted keys; order[i] = the face-edge (3 f + e) key i came from.  counts [3 F] by face-edge; pairs [3 F] by sorted
// position: (face, face) at the first key of a run of two from different faces, (-1, -1) elsewhere.
__global__ void __launch_bounds__(RG_BLOCK) regions_edge_run_kernel(int n, const long long* __restrict__ skeys, const long long* __restrict__ order,
                                                                    int* __restrict__ counts, int2* __restrict__ pairs)
{
    const int i = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (i >= n) return;
    const long long k = skeys[i];
    const int slot = (int)order[i];
    int2 pr = make_int2(-1, -1);
    if (k == RG_SENTINEL) {
        counts[slot] = 0;
        pairs[i] = pr;
        return;
    }
    int lo = i, hi = i + 1;      // the run is [lo, hi)
    for (int s = 0; s < RG_WALK && lo > 0 && skeys[lo - 1] == k; ++s) --lo;
    if (lo > 0 && skeys[lo - 1] == k) {          // a long run: the first position holding k, by bisection over [0, lo)
        int l = 0, r = lo - 1;                   // skeys[r] == k
        while (l < r) {
            const int m = l + (r - l) / 2;
            if (skeys[m] < k) l = m + 1; else r = m;
        }
        lo = l;
    }
    for (int s = 0; s < RG_WALK && hi < n && skeys[hi] == k; ++s) ++hi;
    if (hi < n && skeys[hi] == k) {              // the first position above k, over (hi, n]
        int l = hi + 1, r = n;
        while (l < r) {
            const int m = l + (r - l) / 2;
            if (skeys[m] <= k) l = m + 1; else r = m;
        }
        hi = l;
    }
    counts[slot] = hi - lo;
    if (i == lo && hi - lo == 2) {
        const int fa = (int)(order[lo] / 3), fb = (int)(order[lo + 1] / 3);
        if (fa != fb) pr = make_int2(fa, fb);    // (two face-edges of one degenerate face link nothing)
    }
    pairs[i] = pr;
}

// ---------------------------------------------------------------------------------------------------- components
// (the union-find itself: gsr_unionfind.h)
// scan: the inclusive scan of root_flag.  count must be zero.  One add per wave and label.
__global__ void __launch_bounds__(RG_BLOCK) regions_label_kernel(int F, const int* __restrict__ parent, const int* __restrict__ scan,
                                                                 const unsigned char* __restrict__ sel, int* __restrict__ label,
                                                                 int* __restrict__ count)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    int lab = -1;
    if (f < F) {
        if (sel[f]) lab = scan[parent[f]] - 1;
        label[f] = lab;
    }
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(lab >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int L = __shfl(lab, leader);
        const unsigned long long same = __ballot(lab == L);
        if (lane == leader) atomicAdd(count + L, __popcll(same));
        todo &= ~same;
    }
}

// As a label l = f: a component with more than `thr` faces is region kscan[l] - 1 (kscan: the inclusive scan of count > thr
// over the labels).  As a face: its region, or -1.
__global__ void __launch_bounds__(RG_BLOCK) regions_select_kernel(int F, const int* __restrict__ count, int thr, const int* __restrict__ kscan,
                                                                  const int* __restrict__ label, int cap, int* __restrict__ sel_label,
                                                                  int* __restrict__ sel_count, int* __restrict__ region)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int c = count[f];
    if (c > thr) {
        const int r = kscan[f] - 1;
        if (r < cap) { sel_label[r] = f; sel_count[r] = c; }
    }
    const int lab = label[f];
    region[f] = (lab >= 0 && count[lab] > thr) ? kscan[lab] - 1 : -1;
}

// f32 -> uint32 whose unsigned order is the floats' order
__device__ __forceinline__ unsigned order_bits(float v)
{
    const unsigned u = __float_as_uint(v + 0.f);          // (-0 -> +0)
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(RG_BLOCK) regions_box_init_kernel(int n, unsigned* __restrict__ boxes)
{
    const int i = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (i < n) boxes[i] = (i % 6) < 3 ? 0xffffffffu : 0u;
}

// boxes [cap][2][3] uint32 (order_bits of the min and of the max).  A lane's face gives its own min / max; lanes of equal
// region are combined along the wave (min and max may take the same value twice), and the last lane of each run issues six
// integer atomics.
__global__ void __launch_bounds__(RG_BLOCK) regions_box_kernel(int F, int G, int V, const int* __restrict__ faces, const float* __restrict__ verts,
                                                               const float* __restrict__ points, const int* __restrict__ region, int cap,
                                                               unsigned* __restrict__ boxes, int* __restrict__ err)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    int r = -1;
    unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (f < F) {
        r = region[f];
        if (r >= cap) r = -1;
        if (r >= 0) {
            const int* fv = faces + 3 * (size_t)f;
            for (int k = 0; k < 3; ++k) {
                const int v = fv[k];
                if ((unsigned)v >= (unsigned)V) { atomicOr(err, MESH_ERR_INDEX); continue; }
                for (int a = 0; a < 3; ++a) {
                    const float x = verts[3 * (size_t)v + a];
                    if (x != x) atomicOr(err, MESH_ERR_NAN);
                    const unsigned u = order_bits(x);
                    lo[a] = min(lo[a], u);
                    hi[a] = max(hi[a], u);
                }
            }
            const float* p = points + 3 * (size_t)G * f;
            for (int g = 0; g < G; ++g)
                for (int a = 0; a < 3; ++a) {
                    const float x = p[3 * g + a];
                    if (x != x) atomicOr(err, MESH_ERR_NAN);     // (numpy's min / max would give NaN; the bit order would not)
                    const unsigned u = order_bits(x);
                    lo[a] = min(lo[a], u);
                    hi[a] = max(hi[a], u);
                }
        }
    }
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int rr = __shfl_up(r, d);
        const bool take = lane >= d && rr == r;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned l = __shfl_up(lo[a], d), h = __shfl_up(hi[a], d);
            if (take) { lo[a] = min(lo[a], l); hi[a] = max(hi[a], h); }
        }
    }
    const int next = __shfl_down(r, 1);
    if (r >= 0 && (lane == 63 || next != r)) {
        unsigned* b = boxes + 6 * (size_t)r;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicMin(b + a, lo[a]);
            atomicMax(b + 3 + a, hi[a]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- cut
// find_points_in_boundingbox (:218-224): strictly between the bounds on all three axes, compared in double.
__global__ void __launch_bounds__(RG_BLOCK) regions_inside_kernel(int V, const float* __restrict__ verts, RegionBox box,
                                                                  unsigned char* __restrict__ inside)
{
    const int v = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (v >= V) return;
    bool in = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double x = (double)verts[3 * (size_t)v + a];
        in = in && x > box.lo[a] && x < box.hi[a];
    }
    inside[v] = in;
}

// ref must be zero.  keep: any vertex inside (cut_inner = 0) / no vertex inside (cut_inner = 1).
__global__ void __launch_bounds__(RG_BLOCK) regions_cut_mark_kernel(int F, int V, const int* __restrict__ faces, const unsigned char* __restrict__ inside,
                                                                    int cut_inner, int* __restrict__ keep, int* __restrict__ ref,
                                                                    int* __restrict__ err)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    int v[3];
    if (!mesh_face(faces, f, V, v)) {
        atomicOr(err, MESH_ERR_INDEX);
        keep[f] = 0;
        return;
    }
    const int k = inside[v[0]] + inside[v[1]] + inside[v[2]];
    const int kp = cut_inner ? (k == 0) : (k > 0);
    keep[f] = kp;
    if (kp) { ref[v[0]] = 1; ref[v[1]] = 1; ref[v[2]] = 1; }
}

// kscan / vscan: the inclusive scans of keep / ref.  Kept faces keep their order; referenced vertices are renumbered in
// ascending old index (remove_unreferenced_vertices).
__global__ void __launch_bounds__(RG_BLOCK) regions_cut_faces_kernel(int F, const int* __restrict__ faces, const int* __restrict__ keep,
                                                                     const int* __restrict__ kscan, const int* __restrict__ vscan,
                                                                     int* __restrict__ faces_out, unsigned char* __restrict__ face_mask)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int kp = keep[f];
    face_mask[f] = kp != 0;
    if (!kp) return;
    int* o = faces_out + 3 * (size_t)(kscan[f] - 1);
    o[0] = vscan[faces[3 * (size_t)f]] - 1;
    o[1] = vscan[faces[3 * (size_t)f + 1]] - 1;
    o[2] = vscan[faces[3 * (size_t)f + 2]] - 1;
}

__global__ void __launch_bounds__(RG_BLOCK) regions_cut_verts_kernel(int V, const int* __restrict__ ref, const int* __restrict__ vscan,
                                                                     int* __restrict__ vert_map, int* __restrict__ old_of_new)
{
    const int v = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (v >= V) return;
    const int n = ref[v] ? vscan[v] - 1 : -1;
    vert_map[v] = n;
    if (n >= 0) old_of_new[n] = v;
}

// dst [n_rows][C] = src [old_of_new[row]][C], 4-byte elements, four per thread: one 16-byte store where dst is aligned, one
// 16-byte load too where a row is a whole number of quads (vec bit 0: dst aligned, bit 1: src rows are aligned quads).
__global__ void __launch_bounds__(RG_BLOCK) regions_gather_kernel(long long n_el, int C, const int* __restrict__ old_of_new,
                                                                  const unsigned* __restrict__ src, unsigned* __restrict__ dst, int vec)
{
    const long long q = ((long long)blockIdx.x * RG_BLOCK + threadIdx.x) * 4;
    if (q >= n_el) return;
    long long row = q / C;
    int col = (int)(q - row * C);
    if ((vec & 2) && (vec & 1)) {       // C % 4 == 0: the quad lies in one row
        *reinterpret_cast<uint4*>(dst + q) = *reinterpret_cast<const uint4*>(src + (long long)old_of_new[row] * C + col);
        return;
    }
    unsigned v[4] = {0u, 0u, 0u, 0u};
    const int n = n_el - q < 4 ? (int)(n_el - q) : 4;
    long long base = (long long)old_of_new[row] * C;
    for (int j = 0; j < n; ++j) {
        v[j] = src[base + col];
        if (++col == C && j + 1 < n) { col = 0; ++row; base = (long long)old_of_new[row] * C; }
    }
    if ((vec & 1) && n == 4) {
        *reinterpret_cast<uint4*>(dst + q) = make_uint4(v[0], v[1], v[2], v[3]);
    } else {
        for (int j = 0; j < n; ++j) dst[q + j] = v[j];
    }
}

// ---------------------------------------------------------------------------------------------------- primitives
// find_boundary_verts (:84-111).  bmark [V] (zero before): vertices of face-edges of count exactly 1.  With `inside`: fmark [V]
// (zero before): vertices of faces with some but not all of their vertices inside (:102-109).
__global__ void __launch_bounds__(RG_BLOCK) regions_boundary_kernel(int F, int V, const int* __restrict__ faces, const int* __restrict__ counts,
                                                                    const unsigned char* __restrict__ inside, unsigned char* __restrict__ bmark,
                                                                    unsigned char* __restrict__ fmark, int* __restrict__ err)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    int v[3];
    if (!mesh_face(faces, f, V, v)) { atomicOr(err, MESH_ERR_INDEX); return; }
    for (int e = 0; e < 3; ++e)
        if (counts[3 * (size_t)f + e] == 1) { bmark[v[e]] = 1; bmark[v[(e + 1) % 3]] = 1; }
    if (inside) {
        const int k = inside[v[0]] + inside[v[1]] + inside[v[2]];
        if (k > 0 && k < 3) { fmark[v[0]] = 1; fmark[v[1]] = 1; fmark[v[2]] = 1; }
    }
}

// out[f] = the face's component has at least `min_count` faces (get_outlier_cc_mask, :303-306)
__global__ void __launch_bounds__(RG_BLOCK) regions_label_mask_kernel(int F, const int* __restrict__ label, const int* __restrict__ count,
                                                                      int min_count, unsigned char* __restrict__ out)
{
    const int f = blockIdx.x * RG_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int lab = label[f];
    out[f] = lab >= 0 && count[lab] >= min_count;
}

// gsr_regions_cut_mark: clears the reference flags, then marks
hipError_t launch_regions_cut_mark(int F, int V, const int* faces, const unsigned char* inside, int cut_inner, int* keep, int* ref,
                                   int* err, hipStream_t st)
{
    if (V > 0) {
        const hipError_t e = hipMemsetAsync(ref, 0, sizeof(int) * (size_t)V, st);
        if (e != hipSuccess) return e;
    }
    if (F > 0) regions_cut_mark_kernel<<<mesh_blocks(F), RG_BLOCK, 0, st>>>(F, V, faces, inside, cut_inner, keep, ref, err);
    return hipSuccess;
}

// gsr_regions_boundary: clears the marks, then marks
hipError_t launch_regions_boundary(int F, int V, const int* faces, const int* counts, const unsigned char* inside, unsigned char* bmark,
                                   unsigned char* fmark, int* err, hipStream_t st)
{
    if (V > 0) {
        hipError_t e = hipMemsetAsync(bmark, 0, (size_t)V, st);
        if (e == hipSuccess && inside) e = hipMemsetAsync(fmark, 0, (size_t)V, st);
        if (e != hipSuccess) return e;
    }
    if (F > 0) regions_boundary_kernel<<<mesh_blocks(F), RG_BLOCK, 0, st>>>(F, V, faces, counts, inside, bmark, fmark, err);
    return hipSuccess;
}

}  // namespace

}  // namespace gsr

// ---------------------------------------------------------------- C entry points (include/gsr.h)
using namespace gsr;

extern "C" {

int gsr_regions_edge_keys(int F, const int* faces, const unsigned char* mask, const unsigned char* colour, int cut,
                          unsigned char* selected, long long* keys, int* err, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F)) return fail_msg("gsr_regions_edge_keys: F must be in [0, (2^31 - 1) / 3]");
    if (F == 0) return 0;
    if (!faces || !selected || !keys || !err) return fail_msg("gsr_regions_edge_keys: required pointer is null");
    regions_edge_key_kernel<<<mesh_blocks(F), RG_BLOCK, 0, (hipStream_t)stream>>>(F, faces, mask, colour, cut, selected, keys, err);
    GSR_CHECK_LAUNCH("regions_edge_key_kernel");
    return 0;
}

int gsr_regions_edge_runs(int F, const long long* sorted_keys, const long long* order, int* counts, int* pairs, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F)) return fail_msg("gsr_regions_edge_runs: F must be in [0, (2^31 - 1) / 3]");
    if (F == 0) return 0;
    if (!sorted_keys || !order || !counts || !pairs) return fail_msg("gsr_regions_edge_runs: required pointer is null");
    if (reinterpret_cast<uintptr_t>(pairs) & 7) return fail_msg("gsr_regions_edge_runs: pairs must be 8-byte aligned");
    regions_edge_run_kernel<<<mesh_blocks(3ll * F), RG_BLOCK, 0, (hipStream_t)stream>>>(3 * F, sorted_keys, order, counts,
                                                                                   reinterpret_cast<int2*>(pairs));
    GSR_CHECK_LAUNCH("regions_edge_run_kernel");
    return 0;
}

int gsr_regions_components(int F, const int* pairs, const unsigned char* selected, int* parent, int* root_flag, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F)) return fail_msg("gsr_regions_components: F must be in [0, (2^31 - 1) / 3]");
    if (F == 0) return 0;
    if (!pairs || !selected || !parent || !root_flag) return fail_msg("gsr_regions_components: required pointer is null");
    if (reinterpret_cast<uintptr_t>(pairs) & 7) return fail_msg("gsr_regions_components: pairs must be 8-byte aligned");
    launch_union_find(F, 3ll * F, reinterpret_cast<const int2*>(pairs), selected, parent, root_flag, (hipStream_t)stream);
    GSR_CHECK_LAUNCH("regions union-find kernels");
    return 0;
}

int gsr_regions_labels(int F, const int* parent, const int* root_scan, const unsigned char* selected, int* label, int* count,
                       gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F)) return fail_msg("gsr_regions_labels: F must be in [0, (2^31 - 1) / 3]");
    if (F == 0) return 0;
    if (!parent || !root_scan || !selected || !label || !count) return fail_msg("gsr_regions_labels: required pointer is null");
    regions_label_kernel<<<mesh_blocks(F), RG_BLOCK, 0, (hipStream_t)stream>>>(F, parent, root_scan, selected, label, count);
    GSR_CHECK_LAUNCH("regions_label_kernel");
    return 0;
}

int gsr_regions_select(int F, const int* count, int face_threshold, const int* kept_scan, const int* label, int cap, int* kept_label,
                       int* kept_count, int* region, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || cap < 0) return fail_msg("gsr_regions_select: negative size or too many faces");
    if (face_threshold < 0) return fail_msg("gsr_regions_select: face_threshold must not be negative");
    if (F == 0) return 0;
    if (!count || !kept_scan || !label || !region || (cap > 0 && (!kept_label || !kept_count)))
        return fail_msg("gsr_regions_select: required pointer is null");
    regions_select_kernel<<<mesh_blocks(F), RG_BLOCK, 0, (hipStream_t)stream>>>(F, count, face_threshold, kept_scan, label, cap, kept_label,
                                                                           kept_count, region);
    GSR_CHECK_LAUNCH("regions_select_kernel");
    return 0;
}

int gsr_regions_boxes(int F, int G, int V, const int* faces, const float* verts, const float* points, const int* region, int cap,
                      unsigned int* boxes, int* err, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || G < 0 || V < 0 || cap < 0) return fail_msg("gsr_regions_boxes: negative size or too many faces");
    if (cap == 0) return 0;
    if (!boxes || (F > 0 && (!faces || !verts || !region || !err || (G > 0 && !points))))
        return fail_msg("gsr_regions_boxes: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    regions_box_init_kernel<<<mesh_blocks(6ll * cap), RG_BLOCK, 0, st>>>(6 * cap, boxes);
    if (F > 0) regions_box_kernel<<<mesh_blocks(F), RG_BLOCK, 0, st>>>(F, G, V, faces, verts, points, region, cap, boxes, err);
    GSR_CHECK_LAUNCH("regions box kernels");
    return 0;
}

int gsr_regions_inside(int V, const float* verts, const double* box, unsigned char* inside, gsr_stream_t stream)
{
    clear_error();
    if (V < 0) return fail_msg("gsr_regions_inside: negative size");
    if (!box) return fail_msg("gsr_regions_inside: box is null");
    for (int i = 0; i < 6; ++i)
        if (box[i] != box[i]) return fail_msg("gsr_regions_inside: box holds a NaN");
    if (V == 0) return 0;
    if (!verts || !inside) return fail_msg("gsr_regions_inside: required pointer is null");
    RegionBox b;
    for (int a = 0; a < 3; ++a) { b.lo[a] = box[a]; b.hi[a] = box[3 + a]; }
    regions_inside_kernel<<<mesh_blocks(V), RG_BLOCK, 0, (hipStream_t)stream>>>(V, verts, b, inside);
    GSR_CHECK_LAUNCH("regions_inside_kernel");
    return 0;
}

int gsr_regions_cut_mark(int F, int V, const int* faces, const unsigned char* inside, int cut_inner, int* keep, int* referenced,
                         int* err, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || V < 0) return fail_msg("gsr_regions_cut_mark: negative size or too many faces");
    if ((V > 0 && (!inside || !referenced)) || (F > 0 && (!faces || !keep || !err)))
        return fail_msg("gsr_regions_cut_mark: required pointer is null");
    GSR_CHECK(launch_regions_cut_mark(F, V, faces, inside, cut_inner != 0, keep, referenced, err, (hipStream_t)stream));
    GSR_CHECK_LAUNCH("regions_cut_mark_kernel");
    return 0;
}

int gsr_regions_cut_emit(int F, int V, const int* faces, const int* keep, const int* keep_scan, const int* referenced,
                         const int* referenced_scan, int* faces_out, unsigned char* face_mask, int* vert_map, int* old_of_new,
                         gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || V < 0) return fail_msg("gsr_regions_cut_emit: negative size or too many faces");
    // (faces_out / old_of_new may be null when the scans' totals are zero: nothing is written then)
    if ((F > 0 && (!faces || !keep || !keep_scan || !face_mask || !referenced_scan)) || (V > 0 && (!referenced || !referenced_scan || !vert_map)))
        return fail_msg("gsr_regions_cut_emit: required pointer is null");
    hipStream_t st = (hipStream_t)stream;
    if (F > 0) regions_cut_faces_kernel<<<mesh_blocks(F), RG_BLOCK, 0, st>>>(F, faces, keep, keep_scan, referenced_scan, faces_out, face_mask);
    if (V > 0) regions_cut_verts_kernel<<<mesh_blocks(V), RG_BLOCK, 0, st>>>(V, referenced, referenced_scan, vert_map, old_of_new);
    GSR_CHECK_LAUNCH("regions cut kernels");
    return 0;
}

int gsr_regions_gather(int n_rows, int C, const int* old_of_new, const void* src, void* dst, gsr_stream_t stream)
{
    clear_error();
    if (n_rows < 0 || C < 0) return fail_msg("gsr_regions_gather: negative size");
    if (n_rows == 0 || C == 0) return 0;
    if (!old_of_new || !src || !dst) return fail_msg("gsr_regions_gather: required pointer is null");
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3) return fail_msg("gsr_regions_gather: arrays must be 4-byte aligned");
    const long long n_el = (long long)n_rows * C;
    const int vec = ((reinterpret_cast<uintptr_t>(dst) & 15) == 0 ? 1 : 0) |
                    ((C % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) ? 2 : 0);
    regions_gather_kernel<<<mesh_blocks((n_el + 3) / 4), RG_BLOCK, 0, (hipStream_t)stream>>>(
        n_el, C, old_of_new, static_cast<const unsigned*>(src), static_cast<unsigned*>(dst), vec);
    GSR_CHECK_LAUNCH("regions_gather_kernel");
    return 0;
}

int gsr_regions_boundary(int F, int V, const int* faces, const int* counts, const unsigned char* inside, unsigned char* edge_mark,
                         unsigned char* face_mark, int* err, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F) || V < 0) return fail_msg("gsr_regions_boundary: negative size or too many faces");
    if ((V > 0 && (!edge_mark || (inside && !face_mark))) || (F > 0 && (!faces || !counts || !err)))
        return fail_msg("gsr_regions_boundary: required pointer is null");
    GSR_CHECK(launch_regions_boundary(F, V, faces, counts, inside, edge_mark, face_mark, err, (hipStream_t)stream));
    GSR_CHECK_LAUNCH("regions_boundary_kernel");
    return 0;
}

int gsr_regions_label_mask(int F, const int* label, const int* count, int min_count, unsigned char* out, gsr_stream_t stream)
{
    clear_error();
    if (!mesh_faces_ok(F)) return fail_msg("gsr_regions_label_mask: F must be in [0, (2^31 - 1) / 3]");
    if (F == 0) return 0;
    if (!label || !count || !out) return fail_msg("gsr_regions_label_mask: required pointer is null");
    regions_label_mask_kernel<<<mesh_blocks(F), RG_BLOCK, 0, (hipStream_t)stream>>>(F, label, count, min_count, out);
    GSR_CHECK_LAUNCH("regions_label_mask_kernel");
    return 0;
}

}  // extern "C"
