// gsr_entry.h -- what a C entry point (include/gsr.h) needs on the host: the thread's error string, the launch checks and the
// profiler's brackets.  Every feature's .hip defines its own entry points below its kernels and includes this; the error
// string, the profiler and the stage names themselves are defined once, in gsr_api.hip.
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>

namespace gsr {

// the calling thread's gsr_last_error()
void clear_error();
int fail(const char* where, hipError_t e);   // -> 1; the error reads "<where>: <HIP's message>"
int fail_msg(const char* msg);               // -> 2

#define GSR_CHECK(expr)                                   \
    do {                                                  \
        hipError_t e__ = (expr);                          \
        if (e__ != hipSuccess) return fail(#expr, e__);   \
    } while (0)
#define GSR_CHECK_LAUNCH(name)                            \
    do {                                                  \
        hipError_t e__ = hipGetLastError();               \
        if (e__ != hipSuccess) return fail(name, e__);    \
    } while (0)

// ---- optional per-kernel timing (gsr_profile_*): HIP events on the launch stream around every stage.
enum Stage { ST_PREPROCESS = 0, ST_TILE_SCAN, ST_SCATTER, ST_TILE_SORT, ST_BLEND_FWD, ST_ZERO_FILL, ST_BLEND_BWD,
             ST_GEOM_BWD, ST_LOSS, ST_PRODUCERS, ST_OPTIM, ST_COUNT };
extern std::atomic<bool> g_profiling;   // gsr_profile_enable
struct Scope {
    int stage; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    Scope(int stage_, hipStream_t st_) : stage(stage_), st(st_)   // stage < 0: no bracket
    {
        if (stage >= 0 && g_profiling.load(std::memory_order_relaxed)) open();
    }
    ~Scope() { if (a) close(); }
    void open();    // takes two events and records the first
    void close();   // records the second and files the pair under `stage`
};

}  // namespace gsr
