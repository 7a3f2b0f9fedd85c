// trace_instanced_motion_kernels.hip -- the two-level trace with time-sampled instance transforms, for gfx950
// (ntr_trace_instanced_motion, ntr_trace_instanced_motion_stats; the rule is tests/np_instanced_motion.py):
// trace_instanced_body.h with NTR_TI_MOTION, the masked loop of trace_instanced_masked_kernels.hip and one addition to its entering step.
//   time    per lane, one register through the loop: d_rayTimes[r] or the launch's scalar, clamped to [0, 1] (a NaN gives 0)
//   moving  word 15 of the fetched record, which ntr_tlas_motion_refit (tlas_motion_refit_kernels.hip) sets and no other kernel reads:
//           the record came with the step's one fetch, so a static instance costs no further load
//   pose    motion_pose (trace_motion_pose.h; the arithmetic is instance_motion.h's): the instance's two keys (two 48-byte loads from the motion key buffer at 128 * i, through a range-checked
//           descriptor: beyond the extent they return zeros, and a zero matrix is singular), twelve lerps in binary32 and
//           instance_invert (instance_math.h: binary64, the function ntr_instance_invert and ntr_instances_update use).  Its three rows
//           replace the record's in the registers the fetch wrote, and the masked kernel's transform goes on from there.  No inverse
//           at this time: the step is a pop
//   vote    the pose sits behind __ballot(entering && moving) != 0: a wave that enters only static instances executes the masked
//           kernel's step after one scalar branch; the binary64 registers are live inside the branch only
// Two kernels, trace_instanced_motion and its instrumented variant (counters [12], [13]: moving entries, singular steps), in a unit of
// their own (trace_instanced_kernels.h: why).  Of the host side the unit holds the fill of their parameters, the choice between them
// and the two entry points; the launch around them is trace_instanced_launch.h's, whose fifth client this is.  With
// motion == NULL the entry points hand the call to ntr_trace_instanced_masked / ntr_trace_instanced_stats, which make their launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "instance_math.h"
#include "instance_motion.h"
#include "instanced_bvh.h"
#include "trace_instanced_launch.h"
#include "trace_lane.h"
#include "trace_fetch.h"
#include "trace_instanced_kernels.h"
#include "trace_motion_pose.h"

namespace ntr {
namespace {

// InstancedMotion, the kernels' motion parameters, and motion_pose, the key loads, are trace_motion_pose.h's, shared with the wide unit
#define NTR_TI_PARAMS InstancedParams p, InstancedExtras x, InstancedMotion mo
#define NTR_TI_MASKED 1
#define NTR_TI_SEEDED 0
#define NTR_TI_FAST 0
#define NTR_TI_MOTION 1

#define NTR_TI_KERNEL trace_instanced_motion
#define NTR_TI_STATS 0
#include "trace_instanced_body.h"
#undef NTR_TI_KERNEL
#undef NTR_TI_STATS

#define NTR_TI_KERNEL trace_instanced_motion_stats
#define NTR_TI_STATS 1
#include "trace_instanced_body.h"
#undef NTR_TI_KERNEL
#undef NTR_TI_STATS

#undef NTR_TI_PARAMS
#undef NTR_TI_MASKED
#undef NTR_TI_SEEDED
#undef NTR_TI_FAST
#undef NTR_TI_MOTION

// The unit's launch under the shared path (trace_instanced_launch.h): stats != NULL launches the instrumented kernel.
int trace_instanced_motion_call(const TwoLevelCall& c)
{
    return two_level_trace(c, [&c](DeviceState* ds, hipStream_t s, unsigned int blocks) {
        InstancedParams p{};
        two_level_fill(p, c, ds);
        p.poolNodes = c.poolNodes; p.poolNodesBytes = (uint32_t)c.poolNodesBytes;
        InstancedExtras x{};
        two_level_fill_visibility(x, c, ds);
        InstancedMotion mo{};
        mo.keys = c.motion->d_motionKeys; mo.rayTimes = c.motion->d_rayTimes; mo.time = c.motion->time;
        mo.keysBytes = (uint32_t)std::min<int64_t>(c.motion->motionKeysBytes, kPoolMaxBytes);
        const dim3 grid(blocks), block(64);
        if (c.stats) hipLaunchKernelGGL(trace_instanced_motion_stats, grid, block, 0, s, p, x, mo);
        else hipLaunchKernelGGL(trace_instanced_motion, grid, block, 0, s, p, x, mo);
    });
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" int ntr_trace_instanced_motion(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                          const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                          int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                          int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis,
                                          const NtrInstanceMotion* motion, float* seconds, void* stream)
{
    if (!motion)   // exactly the launch ntr_trace_instanced_masked makes
        return ntr_trace_instanced_masked(numRays, anyHit, d_rays, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records,
                                          numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, seconds,
                                          stream);
    return trace_instanced_motion_call({"ntr_trace_instanced_motion", kTwoLevelBinary, TwoLevelSeed::kNone, nullptr, numRays, anyHit, d_rays, nullptr,
                                        -1, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records, numInstances, d_poolNodes,
                                        poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, nullptr, seconds, stream, nullptr,
                                        nullptr, motion, nullptr});
}

extern "C" int ntr_trace_instanced_motion_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                                                int32_t* d_instanceIDs, const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink,
                                                const void* d_records, int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes,
                                                const void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                                const NtrInstanceVisibility* vis, const NtrInstanceMotion* motion,
                                                NtrInstancedTraceStats* stats, NtrInstancedMotionStats* motionStats, void* stream)
{
    if (motionStats) memset(motionStats, 0, sizeof(*motionStats));
    if (!stats || !motionStats) {
        if (stats) memset(stats, 0, sizeof(*stats));
        return set_error(NTR_ERR_INVALID, "ntr_trace_instanced_motion_stats: null stats");
    }
    if (!motion)   // the masked kernel's instrumented variant: nothing moves, the two motion counters stay zero
        return ntr_trace_instanced_stats(numRays, anyHit, d_rays, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records,
                                         numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, stats,
                                         stream);
    return trace_instanced_motion_call({"ntr_trace_instanced_motion_stats", kTwoLevelBinary, TwoLevelSeed::kNone, nullptr, numRays, anyHit, d_rays,
                                        nullptr, -1, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records, numInstances,
                                        d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, nullptr, nullptr, stream,
                                        stats, nullptr, motion, motionStats});
}
