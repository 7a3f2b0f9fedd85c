// trace_instanced_fast_kernels.hip -- the two-level trace with the FAST slab test, for gfx950 (ntr_trace_instanced_fast,
// ntr_trace_instanced_fast_stats; the rule is tests/np_instanced_fast.py): trace_instanced_body.h with NTR_TI_FAST, the
// masked loop of trace_instanced_masked_kernels.hip -- or, with a seed, the seeded one of trace_instanced_seeded_kernels.hip -- and one
// addition.  The single-level trace decides FAST per BVH on the host (ntr_bvh_validate's flags) and per wave once; here a lane holds the
// world ray on the top level and a different object ray inside every instance, and the flags must be readable by a captured frame:
//   flags   two words on the device, the withheld bits of the top-level tree and of the pool (instanced_validate_kernels.hip), read
//           once per wave by the launch -- a replay sees what the validate before it in the graph wrote
//   nice    per lane: the CURRENT ray may take FAST on its CURRENT level (level_nice, trace_instanced_nice.h: ray_is_nice against the level's granted
//           flags, and the level's FASTDIV).  Set at the start from the world ray, on entering an instance from the object ray, on
//           leaving from the reloaded world ray; wherever it becomes true the three reciprocals are the ray's
//   vote    one ballot per iteration: no live lane with nice == false -> inner_advance<true, 8> / unified_advance<true, 8>, else the
//           <false, 8> instantiations; a scalar branch, no per-lane divergence between the two forms
// FAST equals GENERIC bit for bit in its range (trace_lane.h), so every result word, the instance ids, the status word and the counters
// are the masked / seeded entry point's whatever the flags say -- as long as they grant nothing the buffers do not hold.
// Four kernels: trace_instanced_fast, trace_instanced_fast_seeded and their instrumented variants, in a unit of their own
// (trace_instanced_kernels.h: why).  Of the host side the unit holds the fill of their parameters, the choice among them and the two
// entry points; the launch around them is trace_instanced_launch.h's, shared with the three sibling units.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "instanced_bvh.h"
#include "trace_instanced_launch.h"
#include "trace_lane.h"
#include "trace_instanced_kernels.h"
#include "trace_instanced_nice.h"

namespace ntr {
namespace {

#define NTR_TI_MASKED 1
#define NTR_TI_FAST 1

#define NTR_TI_PARAMS InstancedParams p, InstancedExtras x, InstancedFast f
#define NTR_TI_SEEDED 0
#define NTR_TI_KERNEL trace_instanced_fast
#define NTR_TI_STATS 0
#include "trace_instanced_body.h"
#undef NTR_TI_KERNEL
#undef NTR_TI_STATS
#define NTR_TI_KERNEL trace_instanced_fast_stats
#define NTR_TI_STATS 1
#include "trace_instanced_body.h"
#undef NTR_TI_KERNEL
#undef NTR_TI_STATS
#undef NTR_TI_SEEDED
#undef NTR_TI_PARAMS

#define NTR_TI_PARAMS InstancedParams p, InstancedExtras x, InstancedSeed sd, InstancedFast f
#define NTR_TI_SEEDED 1
#define NTR_TI_KERNEL trace_instanced_fast_seeded
#define NTR_TI_STATS 0
#include "trace_instanced_body.h"
#undef NTR_TI_KERNEL
#undef NTR_TI_STATS
#define NTR_TI_KERNEL trace_instanced_fast_seeded_stats
#define NTR_TI_STATS 1
#include "trace_instanced_body.h"
#undef NTR_TI_KERNEL
#undef NTR_TI_STATS
#undef NTR_TI_SEEDED
#undef NTR_TI_PARAMS

#undef NTR_TI_MASKED
#undef NTR_TI_FAST

// The unit's launch under the shared path (trace_instanced_launch.h): a seed launches a seeded kernel, stats != NULL an instrumented one.
int trace_instanced_fast_call(const TwoLevelCall& c)
{
    return two_level_trace(c, [&c](DeviceState* ds, hipStream_t s, unsigned int blocks) {
        InstancedParams p{};
        two_level_fill(p, c, ds);
        p.poolNodes = c.poolNodes; p.poolNodesBytes = (uint32_t)c.poolNodesBytes;
        InstancedExtras x{};
        two_level_fill_visibility(x, c, ds);
        InstancedFast f{};
        f.flags = c.d_flags;
        InstancedSeed sd{};
        sd.seedResults = c.seedResults; sd.seedInstance = c.seedInstance;
        const dim3 grid(blocks), block(64);
        if (c.seedResults) {
            if (c.stats) hipLaunchKernelGGL(trace_instanced_fast_seeded_stats, grid, block, 0, s, p, x, sd, f);
            else hipLaunchKernelGGL(trace_instanced_fast_seeded, grid, block, 0, s, p, x, sd, f);
        } else {
            if (c.stats) hipLaunchKernelGGL(trace_instanced_fast_stats, grid, block, 0, s, p, x, f);
            else hipLaunchKernelGGL(trace_instanced_fast, grid, block, 0, s, p, x, f);
        }
    });
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" int ntr_trace_instanced_fast(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                        int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs, const void* d_tlasNodes,
                                        int64_t tlasNodesBytes, int32_t rootLink, const void* d_records, int32_t numInstances,
                                        const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                        const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis, const uint32_t* d_flags, float* seconds,
                                        void* stream)
{
    return trace_instanced_fast_call({"ntr_trace_instanced_fast", kTwoLevelBinary, TwoLevelSeed::kOptional, "ntr_instanced_validate", numRays, anyHit,
                                      d_rays, d_seedResults, seedInstance, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records,
                                      numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, d_flags,
                                      seconds, stream, nullptr, nullptr});
}

extern "C" int ntr_trace_instanced_fast_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                              int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs, const void* d_tlasNodes,
                                              int64_t tlasNodesBytes, int32_t rootLink, const void* d_records, int32_t numInstances,
                                              const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                              int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis,
                                              const uint32_t* d_flags, NtrInstancedTraceStats* stats, NtrInstancedFastStats* fastStats,
                                              void* stream)
{
    if (!stats && !fastStats) return set_error(NTR_ERR_INVALID, "ntr_trace_instanced_fast_stats: null stats");   // (one of them: the shared check)
    return trace_instanced_fast_call({"ntr_trace_instanced_fast_stats", kTwoLevelBinary, TwoLevelSeed::kOptional, "ntr_instanced_validate", numRays,
                                      anyHit, d_rays, d_seedResults, seedInstance, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink,
                                      d_records, numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis,
                                      d_flags, nullptr, stream, stats, fastStats});
}
