// trace_launch.h -- host only: the bracket around ONE trace launch of one ray per lane, stated once for trace_wide_kernels.hip and the
// four units of the two-level trace (trace_instanced_launch.h).  The brackets of ntr_api.cpp and ntr_kdtree.cpp hold other things (a
// prediction inside, another status path) and are their own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntr_internal.h"
#include "device_scratch.h"
#include "sched_state.h"
#include "trace_kernels.h"   // the bits of the status word

namespace ntr {

// launch(blocks) enqueues the kernel on `s` over (numRays + 63) / 64 workgroups of 64.
//   seconds != NULL     timed: the stream is drained, the launch lies between two events, *seconds receives their distance, and a
//                       traversal stack overflow that the sticky status word reports is NTR_ERR_OVERFLOW
//   counterWords != 0   instrumented: that many words of ds->stats are zeroed before the launch and copied to `counters` after it (blocks)
template <class Launch>
int launch_trace_rays(const char* fn, DeviceState* ds, hipStream_t s, int32_t numRays, float* seconds, int counterWords,
                      unsigned long long* counters, Launch&& launch)
{
    StreamEvents<2> ev(s);   // the timed bracket
    if (seconds) {
        NTR_HIP(ev.create());
        NTR_HIP(hipStreamSynchronize(s));
        NTR_HIP(ev.record(0));
    }
    if (counterWords) NTR_HIP(hipMemsetAsync(ds->stats, 0, counterWords * sizeof(unsigned long long), s));
    launch((unsigned int)((numRays + 63) / 64));
    NTR_HIP(hipGetLastError());
    if (seconds) {
        NTR_HIP(ev.record(1));
        float ms = 0.0f;
        NTR_HIP(ev.elapsed(0, 1, &ms));
        *seconds = ms * 1e-3f;
        unsigned int bits = 0;
        if (const int rc = status_fetch(ds, s, &bits)) return rc;
        if (bits & NTR_STATUS_STACK_OVERFLOW) return set_error(NTR_ERR_OVERFLOW, "%s: traversal stack overflow", fn);
    }
    if (counterWords) {
        NTR_HIP(hipMemcpyAsync(counters, ds->stats, counterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        NTR_HIP(hipStreamSynchronize(s));
    }
    return NTR_OK;
}

}  // namespace ntr
