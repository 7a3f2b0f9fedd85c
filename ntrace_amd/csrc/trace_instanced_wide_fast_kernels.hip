// trace_instanced_wide_fast_kernels.hip -- the two-level trace over 4-wide trees with the FAST slab test, for gfx950
// (ntr_trace_instanced_wide_fast, ntr_trace_instanced_wide_fast_stats; the rule is tests/np_instanced_wide_fast.py):
// trace_instanced_wide_body.h with NTR_TIW_FAST, the masked loop of trace_instanced_wide_kernels.hip -- or, with a seed, the seeded one
// of trace_instanced_wide_seeded_kernels.hip -- and the one addition that trace_instanced_fast_kernels.hip made to the binary loop
// (DESIGN.md 6w), point for point:
//   flags   two words on the device, the withheld bits of the WIDE top-level tree and of the WIDE pool (ntr_instanced_wide_validate,
//           instanced_validate_kernels.hip), read once per wave by the launch -- a replay sees what the validate before it in the graph
//           wrote.  Not the binary buffers' flags: the all-wide update path (ntr_pool_wide_refit with rewriteRows, ntr_tlas_wide_refit)
//           runs no binary refit and leaves the binary boxes stale
//   nice    per lane: the CURRENT ray may take FAST on its CURRENT level (level_nice, trace_instanced_nice.h).  Set at the start from the
//           world ray, on entering an instance from the object ray, on leaving from the reloaded world ray; wherever it becomes true the
//           three reciprocals are the ray's
//   vote    one ballot per iteration: no live lane with nice == false -> wide_advance<true> / unified_advance<true, 8>, else the <false>
//           instantiations; a scalar branch, no per-lane divergence between the two forms
// FAST equals GENERIC bit for bit in its range (trace_lane.h), so every result word, the instance ids, the status word and the seven
// counters are ntr_trace_instanced_wide's / _wide_seeded's whatever the flags say -- as long as they grant nothing the buffers do not
// hold.  Four kernels: trace_instanced_wide_fast<STATS> and trace_instanced_wide_fast_seeded<STATS>, in a unit of their own
// (trace_instanced_wide_kernels.h: why).  Of the host side the unit holds the fill of their parameters, the choice among them and the two
// entry points; the launch around them is trace_instanced_launch.h's, shared with the three sibling units.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "instanced_wide_bvh.h"
#include "trace_instanced_launch.h"
#include "trace_lane.h"
#include "trace_wide_lane.h"
#include "trace_instanced_wide_kernels.h"
#include "trace_instanced_nice.h"

namespace ntr {
namespace {

#define NTR_TIW_TEMPLATE template <bool STATS>
#define NTR_TIW_FAST 1

#define NTR_TIW_KERNEL trace_instanced_wide_fast
#define NTR_TIW_PARAMS InstancedWideParams p, InstancedFast fl
#define NTR_TIW_SEEDED 0
#include "trace_instanced_wide_body.h"
#undef NTR_TIW_KERNEL
#undef NTR_TIW_PARAMS
#undef NTR_TIW_SEEDED

#define NTR_TIW_KERNEL trace_instanced_wide_fast_seeded
#define NTR_TIW_PARAMS InstancedWideParams p, InstancedWideSeed sd, InstancedFast fl
#define NTR_TIW_SEEDED 1
#include "trace_instanced_wide_body.h"
#undef NTR_TIW_KERNEL
#undef NTR_TIW_PARAMS
#undef NTR_TIW_SEEDED

#undef NTR_TIW_TEMPLATE
#undef NTR_TIW_FAST

// The unit's launch under the shared path (trace_instanced_launch.h): a seed launches a seeded kernel, stats != NULL an instrumented one.
int trace_instanced_wide_fast_call(const TwoLevelCall& c)
{
    return two_level_trace(c, [&c](DeviceState* ds, hipStream_t s, unsigned int blocks) {
        InstancedWideParams p{};
        two_level_fill(p, c, ds);
        p.poolWide = c.poolNodes; p.poolWideBytes = (uint32_t)c.poolNodesBytes;
        two_level_fill_visibility(p, c, ds);
        InstancedFast fl{};
        fl.flags = c.d_flags;
        InstancedWideSeed sd{};
        sd.seedResults = c.seedResults; sd.seedInstance = c.seedInstance;
        const dim3 grid(blocks), block(64);
        if (c.seedResults) {
            if (c.stats) hipLaunchKernelGGL((trace_instanced_wide_fast_seeded<true>), grid, block, 0, s, p, sd, fl);
            else hipLaunchKernelGGL((trace_instanced_wide_fast_seeded<false>), grid, block, 0, s, p, sd, fl);
        } else {
            if (c.stats) hipLaunchKernelGGL((trace_instanced_wide_fast<true>), grid, block, 0, s, p, fl);
            else hipLaunchKernelGGL((trace_instanced_wide_fast<false>), grid, block, 0, s, p, fl);
        }
    });
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" int ntr_trace_instanced_wide_fast(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                             int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs, const void* d_wideTlasNodes,
                                             int64_t wideTlasNodesBytes, int32_t rootLink, const void* d_wideRecords, int32_t numInstances,
                                             const void* d_widePoolNodes, int64_t widePoolNodesBytes, const void* d_poolTriWoop,
                                             int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis,
                                             const uint32_t* d_flags, float* seconds, void* stream)
{
    return trace_instanced_wide_fast_call({"ntr_trace_instanced_wide_fast", kTwoLevelWide, TwoLevelSeed::kOptional, "ntr_instanced_wide_validate",
                                           numRays, anyHit, d_rays, d_seedResults, seedInstance, d_results, d_instanceIDs, d_wideTlasNodes,
                                           wideTlasNodesBytes, rootLink, d_wideRecords, numInstances, d_widePoolNodes, widePoolNodesBytes,
                                           d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, d_flags, seconds, stream, nullptr, nullptr});
}

extern "C" int ntr_trace_instanced_wide_fast_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                                   int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                                   const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                                                   const void* d_wideRecords, int32_t numInstances, const void* d_widePoolNodes,
                                                   int64_t widePoolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                                   const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis, const uint32_t* d_flags,
                                                   NtrInstancedTraceStats* stats, NtrInstancedFastStats* fastStats, void* stream)
{
    if (!stats && !fastStats) return set_error(NTR_ERR_INVALID, "ntr_trace_instanced_wide_fast_stats: null stats");   // (one of them: the shared check)
    return trace_instanced_wide_fast_call({"ntr_trace_instanced_wide_fast_stats", kTwoLevelWide, TwoLevelSeed::kOptional,
                                           "ntr_instanced_wide_validate", numRays, anyHit, d_rays, d_seedResults, seedInstance, d_results,
                                           d_instanceIDs, d_wideTlasNodes, wideTlasNodesBytes, rootLink, d_wideRecords, numInstances,
                                           d_widePoolNodes, widePoolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, d_flags,
                                           nullptr, stream, stats, fastStats});
}
