// trace_instanced_seeded_kernels.hip -- the seeded variants of the two-level trace for gfx950 (ntr_trace_instanced_seeded,
// ntr_trace_instanced_seeded_stats): trace_instanced_body.h, the masked loop of trace_instanced_masked_kernels.hip, started
// from one result record per ray.  The rule is tests/np_instanced_seeded.py: a seed that is a hit gives the ray's tmax; an any-hit ray
// whose seed is a hit never starts; a lane whose traversal accepts nothing stores the seed's four words verbatim and, for a seed that is
// a hit, seedInstance.  Per lane one coalesced 16-byte load beside the ray's 32, and the same load again at the end for the lanes that
// accepted nothing -- nothing of the seed is held in registers through the loop.  The entry points are in trace_instanced_kernels.hip;
// trace_instanced_kernels.h says why the kernels have a unit of their own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "trace_instanced_kernels.h"

namespace ntr {
namespace {

#define NTR_TI_PARAMS InstancedParams p, InstancedExtras x, InstancedSeed sd
#define NTR_TI_MASKED 1
#define NTR_TI_SEEDED 1
#define NTR_TI_FAST 0

#define NTR_TI_KERNEL trace_instanced_seeded
#define NTR_TI_STATS 0
#include "trace_instanced_body.h"
#undef NTR_TI_KERNEL
#undef NTR_TI_STATS

#define NTR_TI_KERNEL trace_instanced_seeded_stats
#define NTR_TI_STATS 1
#include "trace_instanced_body.h"
#undef NTR_TI_KERNEL
#undef NTR_TI_STATS

#undef NTR_TI_PARAMS
#undef NTR_TI_MASKED
#undef NTR_TI_SEEDED
#undef NTR_TI_FAST

}  // namespace

void launch_trace_instanced_seeded(bool stats, unsigned int blocks, hipStream_t stream, const void* params, const void* extras, const void* seed)
{
    InstancedParams p;
    InstancedExtras x;
    InstancedSeed sd;
    memcpy(&p, params, sizeof(p));
    memcpy(&x, extras, sizeof(x));
    memcpy(&sd, seed, sizeof(sd));
    if (stats) hipLaunchKernelGGL(trace_instanced_seeded_stats, dim3(blocks), dim3(64), 0, stream, p, x, sd);
    else hipLaunchKernelGGL(trace_instanced_seeded, dim3(blocks), dim3(64), 0, stream, p, x, sd);
}

}  // namespace ntr
