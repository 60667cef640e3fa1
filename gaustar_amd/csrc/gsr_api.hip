// gsr_api.hip -- the rasterizer's part of the C ABI (include/gsr.h): stage drivers, scratch sizing, error reporting, profiler.
// (Every other feature's entry points live in that feature's .hip, below its kernels: gsr_entry.h.)
// Host-side counterpart of CudaRasterizer::Rasterizer::{forward,backward,markVisible}
// (DGR/cuda_rasterizer/rasterizer_impl.cu:141-153, :198-336, :340-434).
#include "../../include/gsr.h"
#include "gsr_entry.h"
#include "gsr_internal.h"
#include "gsr_plan.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <utility>

using namespace gsr;

namespace gsr { uint64_t* g_trace = nullptr; }

namespace {
thread_local std::string g_err;
thread_local uint32_t g_pinned_seq = 0;
thread_local uint32_t* g_pinned = nullptr;   // pinned, device-mapped landing pad of this thread (ensure_pad)
// what stage 1 of this thread's last view told the host besides its three outputs: the number of PARTS the view's long lists
// are blended in (tile_scan counts them); stage 2 of the same view picks the forward blend's launch shape by it
thread_local struct { int R, maxc, nseg, parts; } g_last_stage1 = {-1, -1, -1, -1};
// words of the pad: [0..3] stage-1 totals, [4] their sequence number (tile_scan); [8] verdict of a planned preprocess, [9] its
// sequence number
constexpr int PAD_WORDS = 64, PAD_VERDICT = 8;
// ---- one helper per small rule of the drivers below
inline int nonneg(int x) { return x > 0 ? x : 0; }
// the next value of a sequence counter that never yields 0 (0 = "nothing yet" wherever such a number is waited for)
template <class Counter> uint32_t next_nonzero(Counter& c)
{
    const uint32_t x = ++c;
    return x ? x : ++c;
}
// Environment switches the driver reads; each is ON unless its value starts with '0'.  Per call (tools/ab_env.py flips them inside
// one process):   GSR_OWN_COUNTERS   the library's self-cleaning counter block (off: the image buffer's counters, a fill per view)
//                 GSR_SORT_IN_BLEND  short lists are sorted inside the forward blend (off: a separate sort kernel)
//                 GSR_REPLAN         a planned view builds the next view's plan (off: a plan lives until a view outgrows it)
//                 GSR_BWD_LIVE       the backward blend's waves leave on the forward's per-(unit, block) flags (off: flags ignored)
// Once per process: GSR_SYNC_SPIN      stage 1 polls the pinned pad for its totals (off: hipStreamSynchronize)
//                   GSR_EARLY_SCATTER  the fused forward queues scatter behind the scan before the host has the totals
bool env_on(const char* name)
{
    const char* e = getenv(name);
    return !(e && e[0] == '0');
}
std::atomic<long long> g_wait_ns{0}, g_waits{0};   // gsr_debug_host_wait

const char* const kStageNames[ST_COUNT] = {"preprocess_kernel", "tile_scan_kernel", "scatter_kernel",
                                           "tile_sort_kernel", "blend_fwd_kernel", "zero_fill", "blend_bwd_kernel",
                                           "geom_bwd_kernel", "loss_kernels", "producer_kernels", "optimizer_kernels"};
struct Rec { int stage; hipEvent_t a, b; };
// Process-wide (PyTorch runs backward on its own autograd thread), guarded by a mutex.
struct Profiler {
    std::mutex mu;
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t get()
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
};
Profiler g_prof;
}  // namespace

// ---- what gsr_entry.h declares: one definition each, for every translation unit's entry points
namespace gsr {
std::atomic<bool> g_profiling{false};
void Scope::open()
{
    a = g_prof.get(); b = g_prof.get();
    (void)hipEventRecord(a, st);
}
void Scope::close()
{
    (void)hipEventRecord(b, st);
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.recs.push_back(Rec{stage, a, b});
}

void clear_error() { g_err.clear(); }
int fail(const char* where, hipError_t e)
{
    g_err = std::string(where) + ": " + hipGetErrorString(e);
    return 1;
}
int fail_msg(const char* msg)
{
    g_err = msg;
    return 2;
}
}  // namespace gsr

extern "C" {

int gsr_abi_version(void) { return 16; }

const char* gsr_last_error(void) { return g_err.c_str(); }

size_t gsr_geom_bytes(int P) { return carve_geom(nullptr, nonneg(P)).bytes; }
size_t gsr_image_bytes(int W, int H) { return carve_image(nullptr, W, H).bytes; }
size_t gsr_binning_bytes_mt(int R, int num_segments, int num_channels)
{
    return carve_bin(nullptr, nonneg(R), nonneg(num_segments), channels_ok(num_channels) ? num_channels : 3).bytes;
}
size_t gsr_binning_bytes(int R, int num_segments) { return gsr_binning_bytes_mt(R, num_segments, 3); }
size_t gsr_grad_scratch_bytes(int P) { return (size_t)48 * (size_t)nonneg(P) + 256; }
size_t gsr_plan_bytes(int W, int H) { return (W > 0 && H > 0) ? carve_plan(nullptr, W, H).bytes : 0; }

// plan_info blocks: GSR_PLAN_INFO_INTS ints of pinned, device-mapped host memory each (the device writes a plan's header there),
// cut from slabs -- a hipHostMalloc per camera would cost a tenth of a millisecond at every camera's first view.
namespace {
std::mutex g_pi_mu;
std::vector<int*> g_pi_free;
}
int* gsr_plan_info_new(void)
{
    std::lock_guard<std::mutex> lk(g_pi_mu);
    if (g_pi_free.empty()) {
        constexpr int PER_SLAB = 512;
        int* slab = nullptr;
        if (hipHostMalloc((void**)&slab, sizeof(int) * GSR_PLAN_INFO_INTS * PER_SLAB,
                          hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        for (int i = PER_SLAB - 1; i >= 0; i--) g_pi_free.push_back(slab + (size_t)i * GSR_PLAN_INFO_INTS);
    }
    int* p = g_pi_free.back();
    g_pi_free.pop_back();
    memset(p, 0, sizeof(int) * GSR_PLAN_INFO_INTS);
    return p;
}
void gsr_plan_info_free(int* plan_info)
{
    if (!plan_info) return;
    std::lock_guard<std::mutex> lk(g_pi_mu);
    g_pi_free.push_back(plan_info);
}

namespace {
// ---- self-cleaning tile counters (gsr_forward_fused only).  The per-(shard, tile) counters and scatter cursors must be
// zero when preprocess starts; carved from the caller's (fresh) image buffer that costs a fill per view -- a 5 us blit
// plus its dispatch in front of a 23 us kernel.  The fused forward instead keeps them in a library-owned block per
// (device, stream) that the forward blend -- the last kernel of the forward, one workgroup per tile -- hands back zeroed.
// `clean` is host-side bookkeeping of that invariant: it is dropped while a call is in flight and only restored once the
// cleaning kernel has been launched (or the block has been re-filled), so any failure in between costs one fill later.
// `busy` makes a block exclusive to ONE call from acquire_counters() until its stage 2 has been launched (or the call
// has bailed out): a second host thread rendering on the same stream meanwhile gets nullptr and falls back to the
// counters in its own image buffer (one fill per view) instead of interleaving its preprocess with this call's scatter.
struct Counters {
    uint32_t* base = nullptr; size_t words = 0; bool clean = false; std::atomic<bool> busy{false};
    // The block: [PLAN_SYNC_WORDS words of the planned forward (the flag of a view that outgrew its plan)] [tile counters of the
    // exact path] [cursor block 0] [cursor block 1].  The sync words come FIRST: where they lie must not depend on the image
    // size -- a flag left behind at a small image's offset would read as a tile count of a larger image's view.
    // The two cursor blocks (round 6; one cursor per tile, PLAN_CURSOR_STRIDE words apart): a planned view claims on one of them
    // and its forward blend leaves the counts standing for the plan job riding in it, while zeroing the tile's cursor in the
    // OTHER block (the previous planned view's).  cur_dirty[b] = number of leading tiles of block b that may be non-zero --
    // host-side bookkeeping like `clean`: a block is only claimed on when it is 0, and a view of T tiles leaves the other
    // block clean up to T (views of different image sizes on one stream cost a fill now and then, never a wrong count).
    size_t cnt_words = 0, cur_words = 0;
    size_t cur_dirty[2] = {0, 0};
    uint32_t* sync() const { return base; }
    uint32_t* cnt() const { return base ? base + PLAN_SYNC_WORDS : nullptr; }
    uint32_t* cursors(int b) const { return base ? base + PLAN_SYNC_WORDS + cnt_words + (b ? cur_words : 0) : nullptr; }
    // *blk = the cursor block a planned view claims on: one that is all zero (block 0 is filled if neither is)
    int claim_clean_cursors(hipStream_t st, int* blk)
    {
        *blk = cur_dirty[0] == 0 ? 0 : cur_dirty[1] == 0 ? 1 : -1;
        if (*blk >= 0) return 0;
        *blk = 0;
        GSR_CHECK(hipMemsetAsync(cursors(0), 0, 4 * cur_dirty[0] * PLAN_CURSOR_STRIDE, st));
        cur_dirty[0] = 0;
        return 0;
    }
    // a planned view of T tiles has claimed on block blk: its counts stand there, its forward blend hands the other block's
    // first T cursors back zeroed
    void settle_cursors(int blk, size_t T)
    {
        cur_dirty[blk] = T;
        if (cur_dirty[blk ^ 1] <= T) cur_dirty[blk ^ 1] = 0;
    }
};
std::mutex g_cnt_mu;
std::map<std::pair<int, hipStream_t>, Counters> g_cnt;

struct CountersLease {   // releases the block on every way out of gsr_forward_fused
    Counters* c;
    ~CountersLease() { if (c) c->busy.store(false, std::memory_order_release); }
};

// -> a zeroed block with room for `cnt_words` counters and two blocks of `cur_words` cursors for (current device, st),
// marked in flight and busy; nullptr: use the image buffer
Counters* acquire_counters(hipStream_t st, size_t cnt_words, size_t cur_words)
{
    int dev = 0;
    if (!env_on("GSR_OWN_COUNTERS") || hipGetDevice(&dev) != hipSuccess) return nullptr;
    Counters* c;
    {
        // (the lease is taken under the lock: gsr_release_stream_state tests `busy` under the same lock before it frees
        // the block and erases the node, so a block can never be freed between the lookup and the exchange)
        std::lock_guard<std::mutex> lk(g_cnt_mu);
        c = &g_cnt[std::make_pair(dev, st)];   // std::map: the address stays valid
        if (c->busy.exchange(true, std::memory_order_acquire)) return nullptr;   // another thread's call owns it right now
    }
    if (c->cnt_words < cnt_words || c->cur_words < cur_words) {
        // (a larger image: the regions move, so everything is laid out and filled anew)
        if (c->base) { (void)hipStreamSynchronize(st); (void)hipFree(c->base); }
        c->base = nullptr; c->words = 0; c->clean = false;
        const size_t cw = std::max(cnt_words, c->cnt_words), uw = std::max(cur_words, c->cur_words);
        const size_t all = PLAN_SYNC_WORDS + cw + 2 * uw;
        if (hipMalloc((void**)&c->base, 4 * all) != hipSuccess) {
            (void)hipGetLastError(); c->base = nullptr; c->cnt_words = c->cur_words = 0; c->busy.store(false); return nullptr;
        }
        c->words = all; c->cnt_words = cw; c->cur_words = uw;
    }
    if (!c->clean) {
        if (hipMemsetAsync(c->base, 0, 4 * c->words, st) != hipSuccess) {
            (void)hipGetLastError(); c->busy.store(false); return nullptr;
        }
        c->cur_dirty[0] = c->cur_dirty[1] = 0;
    }
    c->clean = false;   // in flight
    return c;
}

// Wait for a kernel's word in the pinned pad: normal waits are far below a millisecond and touch nothing but the pad.  The
// stream is only consulted (did it finish or fault?) once a wait has lasted 2 ms, then every 2 ms: hipStreamQuery takes
// runtime locks.  -> 0 and *seen = whether the word showed up (false: the stream retired without it), or an error code.
int wait_pad_word(const volatile uint32_t* flag, uint32_t seq, hipStream_t st, bool* seen)
{
    const auto t_wait0 = std::chrono::steady_clock::now();
    auto next_query = t_wait0 + std::chrono::milliseconds(2);
    for (uint32_t polls = 1; *flag != seq; polls++) {
        if ((polls & 1023u) == 0u && std::chrono::steady_clock::now() >= next_query) {
            const hipError_t q = hipStreamQuery(st);
            if (q == hipSuccess) break;              // kernel retired: its stores are visible
            if (q != hipErrorNotReady) GSR_CHECK(q);   // a fault surfaces here
            next_query = std::chrono::steady_clock::now() + std::chrono::milliseconds(2);
        }
        __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    *seen = *flag == seq;
    g_wait_ns.fetch_add(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_wait0).count(),
                        std::memory_order_relaxed);
    g_waits.fetch_add(1, std::memory_order_relaxed);
    return 0;
}

// The same, for a word whose value also lies in device memory: when the stream retired without the store into the pad showing
// up (never observed, but a platform where device stores to mapped host memory are not coherent must not yield stale values),
// `bytes` from `dev_src` are fetched into `host_dst` with an ordinary copy and the stream is synchronised.
int wait_or_copy_back(const volatile uint32_t* flag, uint32_t seq, hipStream_t st, void* host_dst, const void* dev_src, size_t bytes,
                      bool* seen)
{
    if (const int bad = wait_pad_word(flag, seq, st, seen)) return bad;
    if (*seen) return 0;
    GSR_CHECK(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, st));
    GSR_CHECK(hipStreamSynchronize(st));
    return 0;
}

int ensure_pad()
{
    if (!g_pinned) {
        GSR_CHECK(hipHostMalloc((void**)&g_pinned, 4 * PAD_WORDS, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
        memset(g_pinned, 0, 4 * PAD_WORDS);
    }
    return 0;
}
uint32_t next_seq() { return next_nonzero(g_pinned_seq); }   // (0 is the pad's initial value)
uint32_t next_view_token()
{
    // Token of a view (never 0, unique in the process): a preprocess workgroup that cannot record all of its instances
    // stores it in totals[4], the scan stores it in totals[5], and scatter walks the tiles again iff the two are equal.
    // No word has to be cleared between views, and a stale or uninitialised totals[4] can only select the slower path.
    static std::atomic<uint32_t> g_view_token{0};
    return next_nonzero(g_view_token);
}

// One view's inputs as the entry points receive them, by field name (gsr_internal.h ViewArgs)
ViewArgs view_args(int P, int D, int M, const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                   const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                   const float* viewmatrix, const float* projmatrix, const float* campos, int W, int H, float tan_fovx,
                   float tan_fovy, int* radii)
{
    ViewArgs v;
    v.P = P; v.D = D; v.M = M;
    v.means3D = means3D; v.shs = shs; v.colors_precomp = colors_precomp; v.opacities = opacities;
    v.scales = scales; v.scale_modifier = scale_modifier; v.rotations = rotations; v.cov3D_precomp = cov3D_precomp;
    v.viewmatrix = viewmatrix; v.projmatrix = projmatrix; v.campos = campos;
    v.W = W; v.H = H; v.tan_fovx = tan_fovx; v.tan_fovy = tan_fovy; v.radii = radii;
    return v;
}
// the image buffer's state, with the library's counter block (already zero: acquire_counters; nullptr: none) in place of its own
ImageState carve_image_with(void* image_buffer, int W, int H, uint32_t* counters)
{
    ImageState im = carve_image(image_buffer, W, H);
    if (counters) {
        im.tile_count = counters;
        im.tile_cursor = counters + (size_t)shard_stride(tiles_of(W, H).T) * NSHARD;
    }
    return im;
}
// what the blends read as a Gaussian's colours
const float* features_of(const float* colors_precomp, const GeomState& g) { return colors_precomp ? colors_precomp : g.rgb; }

int check_stage1_args(const ViewArgs& v, const void* geom_buffer, const void* image_buffer)
{
    if ((long long)tiles_of(v.W > 0 ? v.W : 1, v.H > 0 ? v.H : 1).T > 256ll * 1024)
        return fail_msg("gsr_forward_stage1: image too large (more than 262144 tiles)");
    if (v.W <= 0 || v.H <= 0) return fail_msg("gsr_forward_stage1: image size must be positive");
    if (v.P < 0) return fail_msg("gsr_forward_stage1: negative P");
    if (!image_buffer) return fail_msg("gsr_forward_stage1: image_buffer is null");
    if (v.P > 0) {
        if (!v.means3D || !v.opacities || !v.viewmatrix || !v.projmatrix || !v.campos || !v.radii || !geom_buffer)
            return fail_msg("gsr_forward_stage1: required pointer is null");
        if ((v.shs == nullptr) == (v.colors_precomp == nullptr))
            return fail_msg("gsr_forward_stage1: provide exactly one of shs / colors_precomp");
        if (v.shs && (v.D < 0 || v.D > 3 || (v.D + 1) * (v.D + 1) > v.M))
            return fail_msg("gsr_forward_stage1: sh degree must be 0..3 and fit in M coefficients");
        if ((v.cov3D_precomp == nullptr) == (v.scales == nullptr || v.rotations == nullptr))
            return fail_msg("gsr_forward_stage1: provide exactly one of scales+rotations / cov3D_precomp");
    }
    return 0;
}

// (the entry points drop `prefiltered`: the reference only uses it to trap on a culled point, auxiliary.h:156-160)
int forward_stage1_impl(const ViewArgs& v, void* geom_buffer, void* image_buffer, int* num_rendered, int* max_tile_instances,
                        int* num_segments, uint32_t* counters, gsr_stream_t stream, void* early_bin = nullptr,
                        size_t early_capacity = 0, int early_C = 3)
{
    g_err.clear();
    if (!num_rendered || !max_tile_instances || !num_segments)
        return fail_msg("gsr_forward_stage1: null output pointer");
    *num_rendered = 0;
    *max_tile_instances = 0;
    *num_segments = 0;
    if (const int bad = check_stage1_args(v, geom_buffer, image_buffer)) return bad;
    const int P = v.P, W = v.W, H = v.H;
    hipStream_t st = (hipStream_t)stream;
    const Tiles t = tiles_of(W, H);
    ImageState im = carve_image_with(image_buffer, W, H, counters);
    if (!counters) {   // counters and cursors are adjacent in the image buffer: one fill covers both
        GSR_CHECK(hipMemsetAsync(im.tile_count, 0,
                                 (size_t)((char*)(im.tile_cursor + shard_stride(t.T) * NSHARD) - (char*)im.tile_count), st));
    }
    const uint32_t view_token = next_view_token();
    if (P > 0) {
        GeomState g = carve_geom(geom_buffer, P);
        {
            Scope sc(ST_PREPROCESS, st);
            launch_preprocess(v, g, im, view_token, st);
        }
        GSR_CHECK_LAUNCH("preprocess_kernel");
    }
    // Pinned landing pad, mapped into the device's address space: tile_scan stores the four totals and then this call's
    // sequence number into it.  The host polls the sequence word instead of blocking in hipStreamSynchronize (whose
    // interrupt wake-up costs tens of microseconds of idle GPU per view); every few thousand polls it asks the stream
    // whether it finished or faulted, so a failed kernel ends the wait with its error.  GSR_SYNC_SPIN=0 -> plain sync.
    if (const int bad = ensure_pad()) return bad;
    static const bool spin = env_on("GSR_SYNC_SPIN");
    const uint32_t seq = next_seq();
    {
        Scope sc(ST_TILE_SCAN, st);
        launch_tile_scan(im, t.T, g_pinned, seq, view_token, st);
    }
    GSR_CHECK_LAUNCH("tile_scan_kernel");
    if (early_bin && P > 0) {
        // The fused forward already holds a binning buffer: scatter goes out right behind the scan and resolves its
        // pointers from the totals on the device, instead of idling the GPU for the host's round trip (~4.6 us per view).
        {
            Scope sc(ST_SCATTER, st);
            launch_scatter_early(P, W, H, early_C, carve_geom(geom_buffer, P), im, early_bin, early_capacity, st);
        }
        GSR_CHECK_LAUNCH("scatter_kernel");
    }
    if (spin) {
        bool seen = false;
        if (const int bad = wait_or_copy_back(g_pinned + 4, seq, st, g_pinned, im.totals, 16, &seen)) return bad;
        if (!seen) g_pinned[5] = 0xffffffffu;   // (the number of parts did not arrive either: -1 = let stage 2 decide from the sizes)
    } else {
        GSR_CHECK(hipStreamSynchronize(st));   // the forward's single host sync (cf. rasterizer_impl.cu:281)
    }
    *num_rendered = (int)g_pinned[0];
    *max_tile_instances = (int)g_pinned[1];
    *num_segments = (int)g_pinned[3];
    g_last_stage1 = {*num_rendered, *max_tile_instances, *num_segments, spin ? (int)g_pinned[5] : -1};
    return 0;
}

// what stage 2 asks of its arguments, whichever driver launches the forward blend
int check_stage2_args(int R, int num_channels, int W, int H, const float* background, const float* colors_precomp,
                      const void* geom_buffer, const void* binning_buffer, const void* image_buffer, const float* out_color)
{
    if (W <= 0 || H <= 0) return fail_msg("gsr_forward_stage2: image size must be positive");
    if (!background || !out_color || !image_buffer) return fail_msg("gsr_forward_stage2: required pointer is null");
    if (R > 0 && (!binning_buffer || !geom_buffer)) return fail_msg("gsr_forward_stage2: scratch buffer is null");
    if (!channels_ok(num_channels)) return fail_msg("gsr_forward_stage2: num_channels must be 3, 4 or 6");
    if (num_channels != 3 && !colors_precomp)
        return fail_msg("gsr_forward_stage2: multi-target renders need precomputed colours [P, num_channels]");
    return 0;
}

// grad_scratch != nullptr: the backward's accumulation table, cleared by the forward blend on the side (gsr_forward_fused)
int forward_stage2_impl(int P, int R, int max_tile_instances, int num_segments, int num_channels, int W, int H,
                        const float* background, const float* colors_precomp, void* geom_buffer, void* binning_buffer,
                        void* image_buffer, float* out_color, void* grad_scratch, uint32_t* counters, gsr_stream_t stream,
                        bool scattered, const PlanJob* job = nullptr, bool* job_rides = nullptr)
{
    g_err.clear();
    if (const int bad = check_stage2_args(R, num_channels, W, H, background, colors_precomp, geom_buffer, binning_buffer, image_buffer,
                                          out_color))
        return bad;
    const int C = num_channels;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t max_count = (uint32_t)nonneg(max_tile_instances);
    ImageState im = carve_image_with(image_buffer, W, H, counters);   // (the blend hands the library's counters back zeroed)
    GeomState g = carve_geom(geom_buffer, nonneg(P));
    // num_segments < 0: forward-only render (same buffer size as for |num_segments|; the blended-instance words the
    // backward would replay are not written back)
    const bool forward_only = num_segments < 0;
    if (num_segments < 0) num_segments = -num_segments;
    if (R > 0 && num_segments == 0) return fail_msg("gsr_forward_stage2: num_segments of stage 1 is required (it sizes the binning buffer)");
    BinState b = carve_bin(binning_buffer, nonneg(R), num_segments, C);
    bool sort_in_blend = false;
    if (R > 0) {
        if (!scattered) {   // (the fused forward has launched it behind the scan already)
            Scope sc(ST_SCATTER, st);
            launch_scatter(P, W, H, R, max_count, g, im, b, st);
            GSR_CHECK_LAUNCH("scatter_kernel");
        }
        {
            const bool fuse = env_on("GSR_SORT_IN_BLEND");
            // (no event bracket around a stage that launches nothing -- every list of a typical view is sorted inside the
            // forward blend; two back-to-back event records read as ~5 us of "kernel")
            Scope sc(tile_sort_launches(R, max_count, fuse) ? ST_TILE_SORT : -1, st);
            sort_in_blend = launch_tile_sort(W, H, R, num_segments, max_count, im, b, fuse, st);
        }
        GSR_CHECK_LAUNCH("tile_sort_kernel");
    }
    const int num_parts = (g_last_stage1.R == R && g_last_stage1.maxc == max_tile_instances && g_last_stage1.nseg == num_segments)
                              ? g_last_stage1.parts : -1;   // (-1: stage 1 of another view, or of another thread)
    {
        Scope sc(ST_BLEND_FWD, st);
        launch_blend_fwd(C, W, H, nonneg(R), num_segments, max_count, background, features_of(colors_precomp, g), g, im, b, out_color,
                         !forward_only, grad_scratch, grad_scratch ? gsr_grad_scratch_bytes(P) : 0, counters, sort_in_blend, st, job,
                         job_rides, num_parts);
    }
    GSR_CHECK_LAUNCH("blend_fwd_kernel");
    return 0;
}

// ---- gsr_forward_fused / gsr_forward_planned: one call's arguments and what its steps share.  forward_fused_impl (below) reads
// as the sequence of the steps: adopt_arrived_plan, planned_view (plan_job + planned_attempt), exact_view (plan_job, and
// hand_back_counters when the guess was too small).
struct FusedCall {
    const ViewArgs& v; int C, need_backward; const float* background;
    void *geom_buffer, *image_buffer, *binning_buffer; size_t binning_capacity; void* grad_scratch; float* out_color;
    int *num_rendered, *max_tile_instances, *num_segments, *blended;
    void* plan_buffer; gsr_plan_info* pi; int* planned;   // pi: the caller's plan_info block (nullptr: gsr_forward_fused)
    gsr_stream_t stream; hipStream_t st; bool sane, keeps_plan; size_t cnt_words;
    Counters* own;   // the library's counter block, leased to this call (nullptr: the image buffer's counters)

    int level() const { return std::min(std::max(pi->level, 0), 3); }
    // the builder of `job` is on its way: the camera's next call waits for its sequence number in pi->arrived
    void expect(const PlanJob& job, int half) const { pi->pending = (int)job.host_seq; pi->pending_half = half; }

    // The plan an earlier view of this camera left behind: its header arrives in pi->header some tens of microseconds into that
    // view's forward blend; nobody waited for it then.  Normally it is long there.
    int adopt_arrived_plan() const
    {
        bool seen = false;
        if (const int bad = wait_pad_word(reinterpret_cast<volatile uint32_t*>(&pi->arrived), (uint32_t)pi->pending, st, &seen))
            return bad;
        const uint32_t* h = reinterpret_cast<const uint32_t*>(pi->header);
        // (a header that is not this image's -- another size's, or not a header at all -- is no plan)
        if (seen && (h[PH_T] != (uint32_t)v.tiles().T || h[PH_U_CAP] != h[PH_R_CAP] >> 6 || (h[PH_R_CAP] & 63u) != 0u)) seen = false;
        // (nor is one that claims more light tiles than the image has tiles: the forward blend's grid is sized by that count)
        if (seen && h[PLAN_PAD_LIGHT] > h[PH_T]) seen = false;
        pi->state = seen ? (h[PH_VALID] == 1u ? 1 : -1) : 0;
        if (seen) {
            pi->R_cap = (int)h[PH_R_CAP]; pi->U_cap = (int)h[PH_U_CAP]; pi->max_cap = (int)h[PH_MAX_CAP];
            pi->reserved1[PI_LIGHT] = (int)h[PLAN_PAD_LIGHT];   // (the arriving count's own word is the next builder's to write)
            pi->half = pi->pending_half & 1;
        }
        pi->pending = 0;
        return 0;
    }

    // The plan workgroup of THIS view (exact or planned) writes the half of the plan buffer that is not in use (-> that half); its
    // header lands in pi->header and is adopted by the camera's next call (above).
    int plan_job(PlanJob& job) const
    {
        const Tiles t = v.tiles();
        const int half = (pi->half & 1) ^ 1;
        const PlanState pl = carve_plan(plan_buffer, v.W, v.H, half);
        job.enabled = 1u; job.T = t.T; job.gx = t.gx; job.gy = t.gy;
        job.header = pl.header; job.ranges = pl.ranges; job.seg_off = pl.seg_off; job.order = pl.order;
        job.split_from_word = split_from();
        job.level = (uint32_t)level();
        job.host_pad = reinterpret_cast<uint32_t*>(pi->header);
        // (the sequence number belongs to the PLAN, not to the calling thread: a plan_info block may be used from several
        // host threads, and a thread-local counter that happens to equal the block's stale `arrived` would make the next
        // call adopt the OLD header while the device holds the new plan)
        uint32_t seq = (uint32_t)pi->arrived;
        job.host_seq = next_nonzero(seq);
        job.cursor = nullptr;
        // (GSR_PLAN_DIAG builds: the plan being replaced, if the buffer has held one)
        job.prev_ranges = pi->R_cap > 0 ? carve_plan(plan_buffer, v.W, v.H, half ^ 1).ranges : nullptr;
        return half;
    }

    // One planned attempt (gsr_internal.h "planned binning") on cursor block blk: preprocess claims bucket slots and writes the
    // keys, the forward blend is queued right behind it, and the host waits for preprocess's verdict only.  *fit = 0: the view did
    // not fit the plan -- nothing was blended, and the library's counter block is clean again once the queued blend has passed.
    int planned_attempt(int blk, const PlanJob* job, int* fit) const
    {
        *fit = 0;
        g_err.clear();
        if (const int bad = check_stage1_args(v, geom_buffer, image_buffer)) return bad;
        if (const int bad = check_stage2_args(pi->R_cap, C, v.W, v.H, background, v.colors_precomp, geom_buffer, binning_buffer,
                                              image_buffer, out_color))
            return bad;
        if (const int bad = ensure_pad()) return bad;
        ImageState im = carve_image(image_buffer, v.W, v.H);
        GeomState g = carve_geom(geom_buffer, v.P);
        BinState b = carve_bin(binning_buffer, pi->R_cap, pi->U_cap, C);
        const PlanState pl = carve_plan(plan_buffer, v.W, v.H, pi->half & 1);
        PlanRun run;
        run.ranges = pl.ranges; run.seg_off = pl.seg_off; run.order = pl.order;
        run.cursor = own->cursors(blk); run.cursor_other = own->cursors(blk ^ 1); run.sync = own->sync();
        run.keys = b.keys; run.unit_info = b.unit_info; run.im_ranges = im.ranges; run.im_seg_off = im.seg_off;
        run.host_pad = g_pinned + PAD_VERDICT; run.host_seq = next_seq(); run.token = next_view_token();
        run.n_light = (uint32_t)std::min(std::max(pi->reserved1[PI_LIGHT], 0), v.tiles().T);
        {
            Scope sc(ST_PREPROCESS, st);
            launch_preprocess_planned(v, g, im, run, st);
        }
        GSR_CHECK_LAUNCH("preprocess_kernel");
        {
            Scope sc(ST_BLEND_FWD, st);
            launch_blend_fwd_planned(C, v.W, v.H, background, features_of(v.colors_precomp, g), g, im, b, out_color, need_backward != 0,
                                     need_backward ? grad_scratch : nullptr,
                                     need_backward && grad_scratch ? gsr_grad_scratch_bytes(v.P) : 0, run, st, job);
        }
        GSR_CHECK_LAUNCH("blend_fwd_kernel");
        bool seen = false;
        uint32_t flag = 0;   // (the stream has retired when this is read back, so it is final)
        if (const int bad = wait_or_copy_back(g_pinned + PAD_VERDICT + 1, run.host_seq, st, &flag, run.sync + 9 * PLAN_SYNC_STRIDE, 4, &seen))
            return bad;
        *fit = seen ? g_pinned[PAD_VERDICT] == 1u : flag != run.token;
        return 0;
    }

    bool has_usable_plan() const
    {
        return keeps_plan && own && pi->state == 1 && pi->R_cap > 0 && pi->U_cap > 0 && binning_buffer && num_rendered &&
               max_tile_instances && num_segments && (split_from() & 0x80000000u) == 0u &&
               gsr_binning_bytes_mt(pi->R_cap, pi->U_cap, C) <= binning_capacity;
    }

    // Bin and blend the view by its camera's plan.  *blended stays 0: it outgrew the plan, and the exact path renders it (the queued
    // blend leaves the counter block clean) and re-plans, with twice the slack.
    int planned_view() const
    {
        const bool replan = env_on("GSR_REPLAN");
        // the cursor block this view claims on must be all zero; the other one is handed back zeroed by this view's forward blend
        int blk = 0, half = 0, fit = 0;
        if (const int bad = own->claim_clean_cursors(st, &blk)) return bad;
        PlanJob job{};
        if (replan) {
            half = plan_job(job);
            job.cursor = own->cursors(blk);
        }
        if (const int bad = planned_attempt(blk, replan ? &job : nullptr, &fit)) return bad;   // (own stays marked dirty: everything is re-filled on its next use)
        own->settle_cursors(blk, (size_t)v.tiles().T);
        if (!fit) {
            pi->state = 0;
            pi->level = std::min(level() + 1, 3);
            if (planned) *planned = -1;
            return 0;
        }
        if (replan) expect(job, half);
        *num_rendered = pi->R_cap;
        *num_segments = pi->U_cap;
        *max_tile_instances = pi->max_cap;
        *blended = 1;
        if (planned) *planned = 1;
        own->clean = true;   // (the exact path's counters were not touched; the cursor blocks are accounted for above)
        return 0;
    }

    // The guess was too small: the caller allocates exactly and runs stage 2 itself -- over the image buffer's own counters, so
    // they get this call's counts (cursors are still zero) and the library's block is filled again.
    int hand_back_counters() const
    {
        if (!own) return 0;
        ImageState im = carve_image(image_buffer, v.W, v.H);
        GSR_CHECK(hipMemcpyAsync(im.tile_count, own->cnt(), 4 * cnt_words / 2, hipMemcpyDeviceToDevice, st));
        GSR_CHECK(hipMemsetAsync(im.tile_cursor, 0, 4 * cnt_words / 2, st));
        GSR_CHECK(hipMemsetAsync(own->cnt(), 0, 4 * cnt_words / 2, st));
        own->clean = true;
        return 0;
    }

    // Scan + scatter: stage 1, then stage 2 right away if the caller's binning buffer holds the view.
    int exact_view() const
    {
        static const bool early_ok = env_on("GSR_EARLY_SCATTER");
        const bool early = early_ok && sane && binning_buffer != nullptr && binning_capacity > 0;
        uint32_t* const counters = own ? own->cnt() : nullptr;
        const int rc = forward_stage1_impl(v, geom_buffer, image_buffer, num_rendered, max_tile_instances, num_segments, counters, stream,
                                           early ? binning_buffer : nullptr, binning_capacity, C);
        if (rc != 0) return rc;   // (own stays marked dirty: re-filled on its next use)
        // The plan this view leaves behind is built by one extra workgroup of its forward blend (gsr_plan.h).  Nobody waits for
        // it: the header lands in the caller's pinned plan_info block and is adopted by the next call with this plan.  Not built
        // when a plan exists (state 1 was tried first; a misfit has reset it to 0), when the camera is known to be unplannable (-1:
        // the caller asks again by resetting it to 0), when this view's longest list cannot be planned, or when stage 2 is left to
        // the caller.
        PlanJob job{};
        bool job_rides = false;
        int half = 0;
        if (keeps_plan && pi->state == 0) {
            if ((uint32_t)*max_tile_instances + 16u > PLAN_MAX_LIST) pi->state = -1;
            else if (*num_rendered > 0) half = plan_job(job);
        }
        if (gsr_binning_bytes_mt(*num_rendered, *num_segments, C) > binning_capacity || (*num_rendered > 0 && !binning_buffer))
            return hand_back_counters();
        const int rc2 = forward_stage2_impl(v.P, *num_rendered, *max_tile_instances, need_backward ? *num_segments : -*num_segments, C,
                                            v.W, v.H, background, v.colors_precomp, geom_buffer, binning_buffer, image_buffer, out_color,
                                            need_backward ? grad_scratch : nullptr, counters, stream, early, job.enabled ? &job : nullptr,
                                            &job_rides);
        if (rc2 != 0) return rc2;
        *blended = 1;
        if (own) own->clean = true;   // the forward blend zeroes every tile's counters and cursors
        if (job_rides) expect(job, half);
        return 0;
    }
};

int forward_fused_impl(const ViewArgs& v, int num_channels, int need_backward, const float* background, void* geom_buffer,
                       void* image_buffer, void* binning_buffer, size_t binning_capacity, void* grad_scratch, float* out_color,
                       int* num_rendered, int* max_tile_instances, int* num_segments, int* blended, void* plan_buffer,
                       int* plan_info, int* planned, gsr_stream_t stream)
{
    if (!blended) { g_err.clear(); return fail_msg("gsr_forward_fused: null output pointer"); }
    *blended = 0;
    if (planned) *planned = 0;
    if (!channels_ok(num_channels)) { g_err.clear(); return fail_msg("gsr_forward_fused: num_channels must be 3, 4 or 6"); }
    hipStream_t st = (hipStream_t)stream;
    const int T = v.W > 0 && v.H > 0 ? v.tiles().T : 0;
    const bool sane = T > 0 && (long long)T <= 256ll * 1024 && image_buffer && v.P > 0;
    const bool keeps_plan = plan_buffer != nullptr && plan_info != nullptr && sane;
    // the exact path's counters and cursors; a caller that keeps plans: two blocks of one cursor per tile, PLAN_CURSOR_STRIDE words
    // apart, behind them
    const size_t cnt_words = sane ? 2 * (size_t)shard_stride(T) * NSHARD : 0;
    const size_t cur_words = keeps_plan ? (size_t)T * PLAN_CURSOR_STRIDE : 0;
    Counters* own = sane ? acquire_counters(st, cnt_words, cur_words) : nullptr;
    CountersLease lease{own};
    const FusedCall c{v, num_channels, need_backward, background, geom_buffer, image_buffer, binning_buffer, binning_capacity,
                      grad_scratch, out_color, num_rendered, max_tile_instances, num_segments, blended, plan_buffer,
                      reinterpret_cast<gsr_plan_info*>(plan_info), planned, stream, st, sane, keeps_plan, cnt_words, own};
    if (keeps_plan && c.pi->pending != 0)
        if (const int bad = c.adopt_arrived_plan()) return bad;
    if (c.has_usable_plan()) {
        if (const int bad = c.planned_view()) return bad;
        if (*blended) return 0;
    }
    return c.exact_view();
}
}  // namespace

int gsr_debug_host_wait(long long* wait_ns, long long* waits, int reset)
{
    if (wait_ns) *wait_ns = g_wait_ns.load(std::memory_order_relaxed);
    if (waits) *waits = g_waits.load(std::memory_order_relaxed);
    if (reset) { g_wait_ns.store(0); g_waits.store(0); }
    return 0;
}

int gsr_forward_stage1(int P, int D, int M, const float* means3D, const float* shs, const float* colors_precomp,
                       const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                       const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                       const float* campos, int W, int H, float tan_fovx, float tan_fovy, int prefiltered, int* radii,
                       void* geom_buffer, void* image_buffer, int* num_rendered, int* max_tile_instances,
                       int* num_segments, gsr_stream_t stream)
{
    (void)prefiltered;
    const ViewArgs v = view_args(P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp,
                                 viewmatrix, projmatrix, campos, W, H, tan_fovx, tan_fovy, radii);
    return forward_stage1_impl(v, geom_buffer, image_buffer, num_rendered, max_tile_instances, num_segments, nullptr, stream);
}

int gsr_forward_fused(int P, int D, int M, int num_channels, int need_backward, const float* means3D, const float* shs,
                      const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                      const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                      const float* projmatrix, const float* campos, int W, int H, float tan_fovx, float tan_fovy,
                      int prefiltered, const float* background, int* radii, void* geom_buffer, void* image_buffer,
                      void* binning_buffer, size_t binning_capacity, void* grad_scratch, float* out_color,
                      int* num_rendered, int* max_tile_instances, int* num_segments, int* blended, gsr_stream_t stream)
{
    (void)prefiltered;
    const ViewArgs v = view_args(P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp,
                                 viewmatrix, projmatrix, campos, W, H, tan_fovx, tan_fovy, radii);
    return forward_fused_impl(v, num_channels, need_backward, background, geom_buffer, image_buffer, binning_buffer, binning_capacity,
                              grad_scratch, out_color, num_rendered, max_tile_instances, num_segments, blended, nullptr, nullptr,
                              nullptr, stream);
}

int gsr_forward_planned(int P, int D, int M, int num_channels, int need_backward, const float* means3D, const float* shs,
                        const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                        const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                        const float* projmatrix, const float* campos, int W, int H, float tan_fovx, float tan_fovy,
                        int prefiltered, const float* background, int* radii, void* geom_buffer, void* image_buffer,
                        void* binning_buffer, size_t binning_capacity, void* grad_scratch, float* out_color,
                        int* num_rendered, int* max_tile_instances, int* num_segments, int* blended, void* plan_buffer,
                        int* plan_info, int* planned, gsr_stream_t stream)
{
    if (!plan_buffer || !plan_info || !planned) { g_err.clear(); return fail_msg("gsr_forward_planned: null plan pointer"); }
    (void)prefiltered;
    const ViewArgs v = view_args(P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp,
                                 viewmatrix, projmatrix, campos, W, H, tan_fovx, tan_fovy, radii);
    return forward_fused_impl(v, num_channels, need_backward, background, geom_buffer, image_buffer, binning_buffer, binning_capacity,
                              grad_scratch, out_color, num_rendered, max_tile_instances, num_segments, blended, plan_buffer, plan_info,
                              planned, stream);
}

int gsr_forward_stage2(int P, int R, int max_tile_instances, int num_segments, int W, int H, const float* background,
                       const float* colors_precomp, void* geom_buffer, void* binning_buffer, void* image_buffer,
                       float* out_color, gsr_stream_t stream)
{
    return gsr_forward_stage2_mt(P, R, max_tile_instances, num_segments, 3, W, H, background, colors_precomp,
                                 geom_buffer, binning_buffer, image_buffer, out_color, stream);
}

int gsr_forward_stage2_mt(int P, int R, int max_tile_instances, int num_segments, int num_channels, int W, int H,
                          const float* background, const float* colors_precomp, void* geom_buffer, void* binning_buffer,
                          void* image_buffer, float* out_color, gsr_stream_t stream)
{
    return forward_stage2_impl(P, R, max_tile_instances, num_segments, num_channels, W, H, background, colors_precomp,
                               geom_buffer, binning_buffer, image_buffer, out_color, nullptr, nullptr, stream, false);
}

int gsr_forward(gsr_alloc_fn geometry_buffer, gsr_alloc_fn binning_buffer, gsr_alloc_fn image_buffer, void* alloc_ctx,
                int P, int D, int M, const float* background, int W, int H, const float* means3D, const float* shs,
                const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                const float* campos, float tan_fovx, float tan_fovy, int prefiltered, float* out_color, int* radii,
                int* num_rendered, gsr_stream_t stream)
{
    g_err.clear();
    if (!geometry_buffer || !binning_buffer || !image_buffer) return fail_msg("gsr_forward: null allocator callback");
    if (!num_rendered) return fail_msg("gsr_forward: num_rendered is null");
    void* geom = geometry_buffer(alloc_ctx, gsr_geom_bytes(P));
    void* img = image_buffer(alloc_ctx, gsr_image_bytes(W, H));
    if (!geom || !img) return fail_msg("gsr_forward: allocator callback returned null");
    int R = 0, maxc = 0, nseg = 0;
    int rc = gsr_forward_stage1(P, D, M, means3D, shs, colors_precomp, opacities, scales, scale_modifier, rotations,
                                cov3D_precomp, viewmatrix, projmatrix, campos, W, H, tan_fovx, tan_fovy, prefiltered,
                                radii, geom, img, &R, &maxc, &nseg, stream);
    if (rc) return rc;
    void* bin = binning_buffer(alloc_ctx, gsr_binning_bytes(R, nseg));
    if (!bin) return fail_msg("gsr_forward: allocator callback returned null");
    rc = gsr_forward_stage2(P, R, maxc, nseg, W, H, background, colors_precomp, geom, bin, img, out_color, stream);
    *num_rendered = R;
    return rc;
}

int gsr_backward(int P, int D, int M, int R, int num_segments, const float* background, int W, int H,
                 const float* means3D, const float* shs, const float* colors_precomp, const float* scales,
                 float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                 const float* projmatrix, const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                 const void* geom_buffer, const void* binning_buffer, const void* image_buffer, const float* dL_dpix,
                 void* grad_scratch, float* dL_dmean2D, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                 float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, gsr_stream_t stream)
{
    return gsr_backward_mt(P, D, M, R, num_segments, 3, background, W, H, means3D, shs, colors_precomp, scales,
                           scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, campos, tan_fovx, tan_fovy,
                           radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, grad_scratch, dL_dmean2D,
                           dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, 0, stream);
}

int gsr_backward_mt(int P, int D, int M, int R, int num_segments, int num_channels, const float* background, int W,
                    int H, const float* means3D,
                 const float* shs, const float* colors_precomp, const float* scales, float scale_modifier,
                 const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                 const float* campos, float tan_fovx, float tan_fovy, const int* radii, const void* geom_buffer,
                 const void* binning_buffer, const void* image_buffer, const float* dL_dpix, void* grad_scratch,
                 float* dL_dmean2D, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D, float* dL_dcov3D,
                 float* dL_dsh, float* dL_dscale, float* dL_drot, int grad_scratch_zeroed, gsr_stream_t stream)
{
    g_err.clear();
    if (P <= 0) return 0;
    if (W <= 0 || H <= 0) return fail_msg("gsr_backward: image size must be positive");
    if (!means3D || !viewmatrix || !projmatrix || !campos || !radii || !geom_buffer || !image_buffer || !dL_dpix ||
        !background)
        return fail_msg("gsr_backward: required pointer is null");
    if (!grad_scratch || !dL_dmean2D || !dL_dopacity || !dL_dcolor || !dL_dmean3D || (cov3D_precomp && !dL_dcov3D))
        return fail_msg("gsr_backward: required gradient pointer is null");
    if (shs && !dL_dsh) return fail_msg("gsr_backward: dL_dsh is null in SH mode");
    if (!cov3D_precomp && (!scales || !rotations || !dL_dscale || !dL_drot))
        return fail_msg("gsr_backward: scales/rotations and their gradients are required without cov3D_precomp");
    if (R > 0 && !binning_buffer) return fail_msg("gsr_backward: binning_buffer is null");
    if (R > 0 && num_segments <= 0)
        return fail_msg("gsr_backward: num_segments of the forward is required (a forward-only render cannot be differentiated)");
    if (!channels_ok(num_channels)) return fail_msg("gsr_backward: num_channels must be 3, 4 or 6");
    if (gsr_grad_scratch_bytes(P) > (size_t)0xffffffffu)   // (the backward blend addresses the table by 32-bit byte offsets)
        return fail_msg("gsr_backward: more than 89 million Gaussians (the accumulation table must stay below 4 GiB)");
    if (num_channels != 3 && !colors_precomp)
        return fail_msg("gsr_backward: multi-target renders need precomputed colours [P, num_channels]");
    const int C = num_channels;
    hipStream_t st = (hipStream_t)stream;
    ImageState im = carve_image(const_cast<void*>(image_buffer), W, H);
    GeomState g = carve_geom(const_cast<void*>(geom_buffer), P);
    BinState b = carve_bin(const_cast<void*>(binning_buffer), nonneg(R), nonneg(num_segments), C);
    // Zero the packed moment records (the only atomic targets); every output tensor is written outright
    // by geom_bwd (cf. the nine zeroed tensors of rasterize_points.cu:151-159).
    float* grad_acc = static_cast<float*>(grad_scratch);
    if (!grad_scratch_zeroed) {   // otherwise the forward blend cleared it on the side (gsr_forward_fused)
        Scope sc(ST_ZERO_FILL, st);
        GSR_CHECK(hipMemsetAsync(grad_acc, 0, gsr_grad_scratch_bytes(P), st));
    }
    if (R > 0) {
        {
            Scope sc(ST_BLEND_BWD, st);
            launch_blend_bwd(C, W, H, num_segments, background, features_of(colors_precomp, g), g, im, b, dL_dpix, grad_acc, env_on("GSR_BWD_LIVE"), st);
        }
        GSR_CHECK_LAUNCH("blend_bwd_kernel");
    }
    {
        Scope sc(ST_GEOM_BWD, st);
        // (no opacities, and no scales / rotations under cov3D_precomp: launch_geom_bwd; the backward only reads the radii)
        const ViewArgs v = view_args(P, D, M, means3D, shs, colors_precomp, nullptr, cov3D_precomp ? nullptr : scales, scale_modifier,
                                     cov3D_precomp ? nullptr : rotations, cov3D_precomp, viewmatrix, projmatrix, campos, W, H,
                                     tan_fovx, tan_fovy, const_cast<int*>(radii));
        launch_geom_bwd(v, g, C, grad_acc, dL_dmean2D, dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, shs ? dL_dsh : nullptr,
                        cov3D_precomp ? nullptr : dL_dscale, cov3D_precomp ? nullptr : dL_drot, st);
    }
    GSR_CHECK_LAUNCH("geom_bwd_kernel");
    return 0;
}

int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present,
                     gsr_stream_t stream)
{
    (void)projmatrix;   // the reference's frustum test only uses the view matrix (auxiliary.h:154)
    g_err.clear();
    if (P <= 0) return 0;
    if (!means3D || !viewmatrix || !present) return fail_msg("gsr_mark_visible: required pointer is null");
    launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream);
    GSR_CHECK_LAUNCH("mark_visible_kernel");
    return 0;
}

int gsr_release_stream_state(gsr_stream_t stream)
{
    g_err.clear();
    hipStream_t st = (hipStream_t)stream;
    int dev = 0;
    GSR_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_cnt_mu);
    auto it = g_cnt.find(std::make_pair(dev, st));
    if (it == g_cnt.end()) return 0;
    if (it->second.busy.exchange(true)) return fail_msg("gsr_release_stream_state: a forward on this stream is in flight");
    if (it->second.base) { GSR_CHECK(hipStreamSynchronize(st)); GSR_CHECK(hipFree(it->second.base)); }
    g_cnt.erase(it);
    return 0;
}

// ---- gsr_camera_key: the sixteen floats of a view matrix to the host without touching the caller's stream.
namespace {
__global__ void __launch_bounds__(64) camera_key_kernel(const float* __restrict__ m, long long s0, long long s1, uint32_t* __restrict__ pad,
                                                        uint32_t seq)
{
    const int lane = threadIdx.x;
    if (lane < 16) pad[lane] = __float_as_uint(m[(long long)(lane >> 2) * s0 + (long long)(lane & 3) * s1]);
    __threadfence_system();   // (one wave: its wait covers every lane's store)
    if (lane == 0) __hip_atomic_store(&pad[16], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
std::mutex g_key_mu;
std::map<int, hipStream_t> g_key_stream;   // device -> the library's non-blocking side stream
constexpr int PAD_KEY = 32;                // words [32 .. 48] of the thread's pad: the matrix, then its sequence number
}  // namespace

namespace {
thread_local uint32_t g_key_seq = 0;          // sequence number of this thread's read under way (0: none)
thread_local hipStream_t g_key_side = nullptr;
}
int gsr_camera_key_begin(const float* viewmatrix, long long row_stride, long long col_stride)
{
    g_err.clear();
    g_key_seq = 0;
    if (!viewmatrix) return fail_msg("gsr_camera_key: null pointer");
    int dev = 0;
    GSR_CHECK(hipGetDevice(&dev));
    hipStream_t side = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_key_mu);
        auto it = g_key_stream.find(dev);
        if (it == g_key_stream.end()) {
            GSR_CHECK(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
            g_key_stream[dev] = side;
        } else {
            side = it->second;
        }
    }
    if (const int bad = ensure_pad()) return bad;
    static_assert(PAD_KEY + 17 <= PAD_WORDS, "pad");
    const uint32_t seq = next_seq();
    camera_key_kernel<<<1, 64, 0, side>>>(viewmatrix, row_stride, col_stride, g_pinned + PAD_KEY, seq);
    GSR_CHECK_LAUNCH("camera_key_kernel");
    g_key_seq = seq;
    g_key_side = side;
    return 0;
}

int gsr_camera_key_end(unsigned long long* key)
{
    if (!key) { g_err.clear(); return fail_msg("gsr_camera_key: null pointer"); }
    if (g_key_seq == 0u) { g_err.clear(); return fail_msg("gsr_camera_key_end: no read under way on this thread"); }
    const uint32_t seq = g_key_seq;
    g_key_seq = 0;
    bool seen = false;
    if (const int bad = wait_pad_word(g_pinned + PAD_KEY + 16, seq, g_key_side, &seen)) return bad;
    if (!seen) return fail_msg("gsr_camera_key: the kernel retired without its store showing up in the pinned pad");
    // FNV-1a over the sixteen words, then a finaliser (the low bits of a float's pattern are what differs between neighbouring
    // cameras of a rig)
    unsigned long long h = 1469598103934665603ull;
    for (int i = 0; i < 16; i++) {
        uint32_t w = g_pinned[PAD_KEY + i];
        if (w == 0x80000000u) w = 0u;   // -0.0 == 0.0: the same camera
        for (int b = 0; b < 4; b++) { h ^= (w >> (8 * b)) & 0xffu; h *= 1099511628211ull; }
    }
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33;
    *key = h;
    return 0;
}

int gsr_camera_key(const float* viewmatrix, long long row_stride, long long col_stride, unsigned long long* key)
{
    if (!key) { g_err.clear(); return fail_msg("gsr_camera_key: null pointer"); }
    if (const int bad = gsr_camera_key_begin(viewmatrix, row_stride, col_stride)) return bad;
    return gsr_camera_key_end(key);
}

int gsr_debug_preprocess_occupancy(int* exact, int* planned)
{
    gsr::preprocess_occupancy(exact, planned);
    return 0;
}

int gsr_debug_set_bwd_order(const void* device_order)
{
    gsr::g_bwd_order = static_cast<const uint32_t*>(device_order);
    return 0;
}

int gsr_debug_set_trace(void* device_buffer)
{
    gsr::g_trace = static_cast<uint64_t*>(device_buffer);
    return 0;
}

// ---- per-kernel timing --------------------------------------------------------------------------
int gsr_num_stages(void) { return ST_COUNT; }
const char* gsr_stage_name(int stage) { return (stage >= 0 && stage < ST_COUNT) ? kStageNames[stage] : ""; }

int gsr_profile_enable(int on)
{
    g_profiling.store(on != 0);
    return 0;
}

int gsr_profile_read(float* ms, int* counts, int reset)
{
    g_err.clear();
    if (!ms || !counts) return fail_msg("gsr_profile_read: null output pointer");
    for (int i = 0; i < ST_COUNT; i++) { ms[i] = 0.f; counts[i] = 0; }
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (const Rec& r : g_prof.recs) {
        GSR_CHECK(hipEventSynchronize(r.b));
        float t = 0.f;
        GSR_CHECK(hipEventElapsedTime(&t, r.a, r.b));
        ms[r.stage] += t;
        counts[r.stage] += 1;
    }
    if (reset) {
        for (const Rec& r : g_prof.recs) { g_prof.pool.push_back(r.a); g_prof.pool.push_back(r.b); }
        g_prof.recs.clear();
    }
    return 0;
}

// ---- introspection -----------------------------------------------------------------------------
__global__ void export_geom_kernel(int P, const float4* g0, const float4* g1, const float* depth, const float* rgb_in,
                                   float* means2D, float* conic_opacity, float* depths, float* rgb)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const float4 a = g0[i], b = g1[i];
    if (means2D) { means2D[2 * i] = a.x; means2D[2 * i + 1] = a.y; }
    if (conic_opacity) {
        conic_opacity[4 * i] = a.z; conic_opacity[4 * i + 1] = a.w; conic_opacity[4 * i + 2] = b.x;
        conic_opacity[4 * i + 3] = b.y;
    }
    if (depths) depths[i] = depth[i];
    if (rgb) { rgb[3 * i] = rgb_in[3 * i]; rgb[3 * i + 1] = rgb_in[3 * i + 1]; rgb[3 * i + 2] = rgb_in[3 * i + 2]; }
}

int gsr_debug_export(int P, int R, int num_segments, int W, int H, const void* geom_buffer, const void* binning_buffer,
                     const void* image_buffer, float* means2D, float* conic_opacity, float* depths, float* rgb,
                     uint32_t* tile_ranges, uint32_t* point_list, float* final_T, uint32_t* n_contrib,
                     gsr_stream_t stream)
{
    g_err.clear();
    hipStream_t st = (hipStream_t)stream;
    const Tiles t = tiles_of(W, H);
    if (P > 0 && geom_buffer && (means2D || conic_opacity || depths || rgb)) {
        GeomState g = carve_geom(const_cast<void*>(geom_buffer), P);
        export_geom_kernel<<<(P + 255) / 256, 256, 0, st>>>(P, g.g0, g.g1, g.depth, g.rgb, means2D, conic_opacity,
                                                            depths, rgb);
        GSR_CHECK_LAUNCH("export_geom_kernel");
    }
    if (image_buffer) {
        ImageState im = carve_image(const_cast<void*>(image_buffer), W, H);
        const size_t N = (size_t)W * H;
        if (tile_ranges) GSR_CHECK(hipMemcpyAsync(tile_ranges, im.ranges, 8 * (size_t)t.T, hipMemcpyDeviceToDevice, st));
        if (final_T) GSR_CHECK(hipMemcpyAsync(final_T, im.final_T, 4 * N, hipMemcpyDeviceToDevice, st));
        if (n_contrib) GSR_CHECK(hipMemcpyAsync(n_contrib, im.n_contrib, 4 * N, hipMemcpyDeviceToDevice, st));
    }
    if (R > 0 && binning_buffer && point_list) {
        BinState b = carve_bin(const_cast<void*>(binning_buffer), R, nonneg(num_segments));
        GSR_CHECK(hipMemcpyAsync(point_list, b.point_list, 4 * (size_t)R, hipMemcpyDeviceToDevice, st));
    }
    return 0;
}

__global__ void export_units_kernel(int U, const uint4* __restrict__ table, uint32_t* __restrict__ unit_info, uint8_t* __restrict__ unit_live)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= U) return;
    const uint4 v = table[i];
    if (unit_info) {
        unit_info[4 * i] = v.x & UNIT_TILE_MASK; unit_info[4 * i + 1] = v.y; unit_info[4 * i + 2] = v.z; unit_info[4 * i + 3] = v.w;
    }
    if (unit_live)
        for (int blk = 0; blk < 4; blk++) unit_live[4 * i + blk] = (uint8_t)((v.x >> (UNIT_LIVE_SHIFT + blk)) & 1u);
}

int gsr_debug_export_units(int R, int num_segments, const void* binning_buffer, uint32_t* unit_info, uint8_t* unit_live,
                           gsr_stream_t stream)
{
    g_err.clear();
    if (R <= 0 || num_segments <= 0) return 0;
    if (!binning_buffer) return fail_msg("gsr_debug_export_units: required pointer is null");
    BinState b = carve_bin(const_cast<void*>(binning_buffer), R, num_segments);
    export_units_kernel<<<(num_segments + 255) / 256, 256, 0, (hipStream_t)stream>>>(num_segments, b.unit_info, unit_info, unit_live);
    GSR_CHECK_LAUNCH("export_units_kernel");
    return 0;
}

int gsr_debug_export_masks(int R, int num_segments, const void* binning_buffer, uint64_t* masks, gsr_stream_t stream)
{
    g_err.clear();
    if (R <= 0 || num_segments <= 0) return 0;
    if (!binning_buffer || !masks) return fail_msg("gsr_debug_export_masks: required pointer is null");
    BinState b = carve_bin(const_cast<void*>(binning_buffer), R, num_segments);
    GSR_CHECK(hipMemcpyAsync(masks, b.masks, 8 * 256 * (size_t)num_segments, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
