// trace_instanced_wide_motion_kernels.hip -- the two-level trace over 4-wide trees with time-sampled instance transforms, for gfx950
// (ntr_trace_instanced_wide_motion, ntr_trace_instanced_wide_motion_stats; the rule is
// tests/np_instanced_wide_motion.py): trace_instanced_wide_body.h with NTR_TIW_MOTION, the masked loop of
// trace_instanced_wide_kernels.hip and one addition to its entering step -- the one trace_instanced_motion_kernels.hip makes to the
// binary loop, in the same place, after the marker-room check.
//   time    per lane, one register through the loop: d_rayTimes[r] or the launch's scalar, clamped to [0, 1] (a NaN gives 0)
//   moving  word 15 of the fetched wide record, which ntr_tlas_wide_motion_refit (tlas_wide_motion_refit_kernels.hip) sets and no
//           other kernel reads (instanced_wide_bvh.h): the record came with the step's one fetch, so a static instance costs no
//           further load
//   pose    motion_pose (trace_motion_pose.h, shared with the binary unit; the arithmetic is instance_motion.h's): the instance's two
//           keys from the motion key buffer at 128 * i, through a range-checked descriptor built from kernel arguments -- beyond the
//           extent they return zeros, and a zero matrix is singular -- twelve lerps in binary32 and instance_invert (binary64).  Its
//           three rows replace the record's in the registers the fetch wrote, and the wide kernel's transform goes on from there.  No
//           inverse at this time: the step is a pop, counted in numSingular only
//   vote    the pose sits behind __ballot(entering && moving) != 0: a wave that enters only static instances executes the masked
//           kernel's step after one scalar branch; the binary64 registers are live inside the branch only
// Two kernels, trace_instanced_wide_motion<false> and its instrumented variant <true> (counters [12], [13]: moving entries, singular
// steps), in a unit of their own (trace_instanced_wide_kernels.h: why).  Of the host side the unit holds the fill of their parameters,
// the choice between them and the two entry points; the launch around them is trace_instanced_launch.h's, whose sixth client this is
// (DESIGN.md 6y).  With motion == NULL the entry points hand the call to ntr_trace_instanced_wide / ntr_trace_instanced_wide_stats, which
// make their launch.  Not here: the seeded / world form and FAST.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "ntr_internal.h"
#include "instance_math.h"
#include "instance_motion.h"
#include "instanced_wide_bvh.h"
#include "trace_instanced_launch.h"
#include "trace_lane.h"
#include "trace_wide_lane.h"
#include "trace_instanced_wide_kernels.h"
#include "trace_motion_pose.h"

namespace ntr {
namespace {

#define NTR_TIW_TEMPLATE template <bool STATS>
#define NTR_TIW_KERNEL trace_instanced_wide_motion
#define NTR_TIW_PARAMS InstancedWideParams p, InstancedMotion mo
#define NTR_TIW_SEEDED 0
#define NTR_TIW_FAST 0
#define NTR_TIW_MOTION 1
#include "trace_instanced_wide_body.h"
#undef NTR_TIW_TEMPLATE
#undef NTR_TIW_KERNEL
#undef NTR_TIW_PARAMS
#undef NTR_TIW_SEEDED
#undef NTR_TIW_FAST
#undef NTR_TIW_MOTION

// The unit's launch under the shared path (trace_instanced_launch.h): stats != NULL launches the instrumented kernel.
int trace_instanced_wide_motion_call(const TwoLevelCall& c)
{
    return two_level_trace(c, [&c](DeviceState* ds, hipStream_t s, unsigned int blocks) {
        InstancedWideParams p{};
        two_level_fill(p, c, ds);
        p.poolWide = c.poolNodes; p.poolWideBytes = (uint32_t)c.poolNodesBytes;
        two_level_fill_visibility(p, c, ds);
        InstancedMotion mo{};
        mo.keys = c.motion->d_motionKeys; mo.rayTimes = c.motion->d_rayTimes; mo.time = c.motion->time;
        mo.keysBytes = (uint32_t)std::min<int64_t>(c.motion->motionKeysBytes, kPoolMaxBytes);
        const dim3 grid(blocks), block(64);
        if (c.stats) hipLaunchKernelGGL((trace_instanced_wide_motion<true>), grid, block, 0, s, p, mo);
        else hipLaunchKernelGGL((trace_instanced_wide_motion<false>), grid, block, 0, s, p, mo);
    });
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" int ntr_trace_instanced_wide_motion(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                                               int32_t* d_instanceIDs, const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                                               const void* d_wideRecords, int32_t numInstances, const void* d_widePoolNodes,
                                               int64_t widePoolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                               const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis, const NtrInstanceMotion* motion,
                                               float* seconds, void* stream)
{
    if (!motion)   // exactly the launch ntr_trace_instanced_wide makes
        return ntr_trace_instanced_wide(numRays, anyHit, d_rays, d_results, d_instanceIDs, d_wideTlasNodes, wideTlasNodesBytes, rootLink,
                                        d_wideRecords, numInstances, d_widePoolNodes, widePoolNodesBytes, d_poolTriWoop, poolTriWoopBytes,
                                        d_poolTriIndex, vis, seconds, stream);
    return trace_instanced_wide_motion_call({"ntr_trace_instanced_wide_motion", kTwoLevelWide, TwoLevelSeed::kNone, nullptr, numRays, anyHit, d_rays,
                                             nullptr, -1, d_results, d_instanceIDs, d_wideTlasNodes, wideTlasNodesBytes, rootLink, d_wideRecords,
                                             numInstances, d_widePoolNodes, widePoolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex,
                                             vis, nullptr, seconds, stream, nullptr, nullptr, motion, nullptr});
}

extern "C" int ntr_trace_instanced_wide_motion_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                                                     int32_t* d_instanceIDs, const void* d_wideTlasNodes, int64_t wideTlasNodesBytes,
                                                     int32_t rootLink, const void* d_wideRecords, int32_t numInstances,
                                                     const void* d_widePoolNodes, int64_t widePoolNodesBytes, const void* d_poolTriWoop,
                                                     int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis,
                                                     const NtrInstanceMotion* motion, NtrInstancedTraceStats* stats,
                                                     NtrInstancedMotionStats* motionStats, void* stream)
{
    if (motionStats) memset(motionStats, 0, sizeof(*motionStats));
    if (!stats || !motionStats) {
        if (stats) memset(stats, 0, sizeof(*stats));
        return set_error(NTR_ERR_INVALID, "ntr_trace_instanced_wide_motion_stats: null stats");
    }
    if (!motion)   // the wide kernel's instrumented variant: nothing moves, the two motion counters stay zero
        return ntr_trace_instanced_wide_stats(numRays, anyHit, d_rays, d_results, d_instanceIDs, d_wideTlasNodes, wideTlasNodesBytes, rootLink,
                                              d_wideRecords, numInstances, d_widePoolNodes, widePoolNodesBytes, d_poolTriWoop, poolTriWoopBytes,
                                              d_poolTriIndex, vis, stats, stream);
    return trace_instanced_wide_motion_call({"ntr_trace_instanced_wide_motion_stats", kTwoLevelWide, TwoLevelSeed::kNone, nullptr, numRays, anyHit,
                                             d_rays, nullptr, -1, d_results, d_instanceIDs, d_wideTlasNodes, wideTlasNodesBytes, rootLink,
                                             d_wideRecords, numInstances, d_widePoolNodes, widePoolNodesBytes, d_poolTriWoop, poolTriWoopBytes,
                                             d_poolTriIndex, vis, nullptr, nullptr, stream, stats, nullptr, motion, motionStats});
}
