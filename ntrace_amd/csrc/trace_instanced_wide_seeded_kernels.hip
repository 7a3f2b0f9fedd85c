// trace_instanced_wide_seeded_kernels.hip -- the seeded variants of the two-level trace over 4-wide trees for gfx950
// (ntr_trace_instanced_wide_seeded, ntr_trace_instanced_wide_seeded_stats): trace_instanced_wide_body.h, the masked loop of
// trace_instanced_wide_kernels.hip, started from one result record per ray.  The rule is tests/np_instanced_seeded.py (trace_wide), the
// same change as in the binary two-level trace (trace_instanced_seeded_kernels.hip): a seed that is a hit gives the ray's tmax; an
// any-hit ray whose seed is a hit never starts; a lane whose traversal accepts nothing stores the seed's four words verbatim and, for a
// seed that is a hit, seedInstance.  The entry points are in trace_instanced_wide_kernels.hip; trace_instanced_wide_kernels.h says why
// the kernels have a unit of their own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "trace_instanced_wide_kernels.h"

namespace ntr {
namespace {

#define NTR_TIW_TEMPLATE template <bool STATS>
#define NTR_TIW_KERNEL trace_instanced_wide_seeded
#define NTR_TIW_PARAMS InstancedWideParams p, InstancedWideSeed sd
#define NTR_TIW_SEEDED 1
#define NTR_TIW_FAST 0
#include "trace_instanced_wide_body.h"
#undef NTR_TIW_TEMPLATE
#undef NTR_TIW_KERNEL
#undef NTR_TIW_PARAMS
#undef NTR_TIW_SEEDED
#undef NTR_TIW_FAST

}  // namespace

void launch_trace_instanced_wide_seeded(bool stats, unsigned int blocks, hipStream_t stream, const void* params, const void* seed)
{
    InstancedWideParams p;
    InstancedWideSeed sd;
    memcpy(&p, params, sizeof(p));
    memcpy(&sd, seed, sizeof(sd));
    if (stats) hipLaunchKernelGGL((trace_instanced_wide_seeded<true>), dim3(blocks), dim3(64), 0, stream, p, sd);
    else hipLaunchKernelGGL((trace_instanced_wide_seeded<false>), dim3(blocks), dim3(64), 0, stream, p, sd);
}

}  // namespace ntr
