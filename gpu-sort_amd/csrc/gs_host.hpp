// gs_host.hpp -- host-side declarations shared by the translation units of
// libgpusort.so.  The public C ABI is include/gpusort.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gpusort.h"

#include <vector>

// Per-kernel event timing (see gs_profile_* in gpusort.h).  KernelTimer brackets
// one launch with an event pair when a profile is bound to this thread; it is a
// no-op (two pointer compares) otherwise.
struct gs_profile {
    struct Span { int id; hipEvent_t a, b; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> pool;
    double ms[GS_K_COUNT] = {0};
    uint64_t launches[GS_K_COUNT] = {0};
};

// Entry points report launch failures through hipGetLastError(), which is per host thread and also holds whatever
// an EARLIER HIP call of the caller (another library, the framework) left behind: drop that first, so that only
// this call's own errors are reported.
#define GS_CLEAR_STALE_ERROR() ((void)hipGetLastError())

// The workspace contract (include/gpusort.h): d_temp may have any alignment.  Every public *_temp_bytes adds GS_WS_SLACK
// once, and every public function that takes d_temp carves its layout from gs_ws_base(d_temp), d_temp rounded up to
// GS_WS_ALIGN bytes (cub's AliasTemporaries does the same).  A function that hands part of its workspace to another public
// one passes an aligned sub-workspace sized by that function's public query.
constexpr size_t GS_WS_ALIGN = 256;
constexpr size_t GS_WS_SLACK = GS_WS_ALIGN;   // (not 255: the queries stay multiples of 256)
static inline char *gs_ws_base(void *d_temp)
{
    return (char *)(((uintptr_t)d_temp + (GS_WS_ALIGN - 1)) & ~(uintptr_t)(GS_WS_ALIGN - 1));
}
// a carve's step: `bytes` rounded up to GS_WS_ALIGN
static inline size_t gs_ws_align(size_t bytes) { return (bytes + (GS_WS_ALIGN - 1)) & ~(GS_WS_ALIGN - 1); }

// Do two byte ranges share a byte?  A null or empty range shares none.
static inline bool gs_ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes)
{
    if (!a || !b || !abytes || !bbytes) return false;
    const char *p = (const char *)a, *q = (const char *)b;
    return p < q + bbytes && q < p + abytes;
}
// Do any two of a call's four arrays (keys in, values in, keys out, values out) overlap?
static inline bool gs_any_overlap4(const void *const arr[4], const size_t bytes[4])
{
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (gs_ranges_overlap(arr[i], bytes[i], arr[j], bytes[j])) return true;
    return false;
}

namespace gs {
extern thread_local gs_profile *tl_profile;

struct KernelTimer {
    gs_profile *p;
    hipStream_t s;
    gs_profile::Span span;
    KernelTimer(int id, hipStream_t stream);
    ~KernelTimer();
};
// Zero `bytes` (a multiple of 8, at an 8-byte aligned address) with a kernel.  Used instead of hipMemsetAsync
// everywhere a sort may be captured in a HIP graph: the memset node of a captured graph was seen not to take
// effect from the second replay on (counters kept growing until the task lists overflowed); a kernel node does.
hipError_t zero_async(void *p, size_t bytes, hipStream_t s);
}  // namespace gs
