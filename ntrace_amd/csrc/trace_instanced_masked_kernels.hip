// trace_instanced_masked_kernels.hip -- the masked and the instrumented variant of the two-level trace for gfx950
// (ntr_trace_instanced_masked, ntr_trace_instanced_stats): trace_instanced_body.h, the loop of trace_instanced_kernels.hip,
// with the entering step asking the instance and ray masks, and with per-lane counters.  The entry points are in trace_instanced_kernels.hip;
// trace_instanced_kernels.h says why the kernels have a unit of their own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "trace_instanced_kernels.h"

namespace ntr {
namespace {

#define NTR_TI_PARAMS InstancedParams p, InstancedExtras x
#define NTR_TI_MASKED 1
#define NTR_TI_SEEDED 0
#define NTR_TI_FAST 0

#define NTR_TI_KERNEL trace_instanced_masked
#define NTR_TI_STATS 0
#include "trace_instanced_body.h"
#undef NTR_TI_KERNEL
#undef NTR_TI_STATS

#define NTR_TI_KERNEL trace_instanced_stats
#define NTR_TI_STATS 1
#include "trace_instanced_body.h"
#undef NTR_TI_KERNEL
#undef NTR_TI_STATS

#undef NTR_TI_PARAMS
#undef NTR_TI_MASKED
#undef NTR_TI_SEEDED
#undef NTR_TI_FAST

}  // namespace

void launch_trace_instanced_variant(bool stats, unsigned int blocks, hipStream_t stream, const void* params, const void* extras)
{
    InstancedParams p;
    InstancedExtras x;
    memcpy(&p, params, sizeof(p));
    memcpy(&x, extras, sizeof(x));
    if (stats) hipLaunchKernelGGL(trace_instanced_stats, dim3(blocks), dim3(64), 0, stream, p, x);
    else hipLaunchKernelGGL(trace_instanced_masked, dim3(blocks), dim3(64), 0, stream, p, x);
}

}  // namespace ntr
