// gsr_unionfind.h -- connected components of n nodes under a list of pairs, by a lock-free union-find: what gsr_regions.hip
// runs over faces (pairs = adjacent faces) and gsr_stitch.hip over vertices (pairs = hole edges).
//
// The larger root is pointed at the smaller by compare-and-swap, so a tree's root is its smallest node whatever order the hooks
// landed in; flatten finds it without a store to any other node's word and writes it to parent[x], once.  Workgroups on
// different XCDs hook concurrently: every read of `parent` inside a find is an agent-scope atomic load, every write an
// agent-scope atomic store or compare-and-swap.
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

namespace {

constexpr int UF_BLOCK = 256;

__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void uf_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(UF_BLOCK) uf_init_kernel(int n, int* __restrict__ parent)
{
    const int x = blockIdx.x * UF_BLOCK + threadIdx.x;
    if (x < n) parent[x] = x;
}

// The root of x, halving the path on the way: for the HOOK kernel only, where any ancestor is as good as another.
// parent[x] <= x always; a node that has a parent below itself never becomes a root again, so the halving store (to an
// ancestor, of a non-root) and the hooks' compare-and-swap (on roots only) never meet on one word.
__device__ __forceinline__ int uf_find(int* parent, int x)
{
    for (;;) {
        const int p = uf_load(parent + x);
        if (p == x) return x;
        const int g = uf_load(parent + p);
        if (g == p) return p;
        uf_store(parent + x, g);
        x = g;
    }
}

// The root of x without a store: for the FLATTEN kernel, where parent[x] must end as the final root.  There every word has one
// writer, the thread of its own node, and the one value it writes is the root; a reader meets either the entry the hooks left
// (an ancestor) or that root, and walks on until parent[x] == x.  No hook runs any more, so roots stay roots.
__device__ __forceinline__ int uf_root(const int* parent, int x)
{
    for (;;) {
        const int p = uf_load(parent + x);
        if (p == x) return x;
        x = p;
    }
}

// pairs [n_pairs]: (a, b) links a and b; (-1, -1) links nothing
__global__ void __launch_bounds__(UF_BLOCK) uf_hook_kernel(long long n_pairs, const int2* __restrict__ pairs, int* __restrict__ parent)
{
    const long long i = (long long)blockIdx.x * UF_BLOCK + threadIdx.x;
    if (i >= n_pairs) return;
    const int2 pr = pairs[i];
    if (pr.x < 0) return;
    int a = pr.x, b = pr.y;
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) break;
        if (a < b) { const int t = a; a = b; b = t; }       // a: the larger root, pointed at the smaller
        const int old = atomicCAS(parent + a, a, b);
        if (old == a) break;
        a = old;                                            // someone hooked a first: go on from where it points
    }
}

__global__ void __launch_bounds__(UF_BLOCK) uf_flatten_kernel(int n, const unsigned char* __restrict__ sel, int* __restrict__ parent,
                                                              int* __restrict__ root_flag)
{
    const int x = blockIdx.x * UF_BLOCK + threadIdx.x;
    if (x >= n) return;
    const int r = uf_root(parent, x);
    uf_store(parent + x, r);      // (the only store to this word in this kernel)
    root_flag[x] = (sel[x] && r == x) ? 1 : 0;
}

// parent [n] = the smallest node of every node's component; root_flag [n] = 1 for the selected nodes that are their own root.
// n > 0, n_pairs >= 0; every pair's ends are in [0, n) or it is (-1, -1).
inline void launch_union_find(int n, long long n_pairs, const int2* pairs, const unsigned char* sel, int* parent, int* root_flag,
                              hipStream_t st)
{
    const unsigned nb = (unsigned)((n + UF_BLOCK - 1) / UF_BLOCK);
    uf_init_kernel<<<nb, UF_BLOCK, 0, st>>>(n, parent);
    if (n_pairs > 0) uf_hook_kernel<<<(unsigned)((n_pairs + UF_BLOCK - 1) / UF_BLOCK), UF_BLOCK, 0, st>>>(n_pairs, pairs, parent);
    uf_flatten_kernel<<<nb, UF_BLOCK, 0, st>>>(n, sel, parent, root_flag);
}

}  // namespace

}  // namespace gsr
