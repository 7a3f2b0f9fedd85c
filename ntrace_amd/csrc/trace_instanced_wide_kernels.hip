// trace_instanced_wide_kernels.hip -- the two-level trace over 4-wide trees for gfx950 (ntr_trace_instanced_wide,
// ntr_trace_instanced_wide_stats): a wide top-level tree over instances, each a wide tree of a wide pool plus a transform
// (instanced_wide_bvh.h).  EXTENSION: the reference has neither instancing nor wide trees; the rule is the numpy spec
// tests/np_instanced_wide.py, which the kernels equal in all four result words, the instance id and every counter.  KNOWN LIMIT, as the
// spec states it: the records may differ from the binary two-level trace's on the same scene (a rounded box test is not conservative and
// the visiting order decides among hits of equal t).  The spec is the definition.
// One loop, 64-thread workgroups, one ray per lane: a unified-step loop built from trace_lane.h.  It joins two kernels:
//   from the two-level body (trace_instanced_body.h)   one stack (16 LDS + 88 scratch entries), the exit marker, the ray transform on
//               entering, one shrinking tmax, the range-checked record fetch, the mask word fetched beside the record and waited for by
//               the same s_waitcnt, the world ray reloaded on leaving
//   from trace_wide_kernels.hip (trace_wide_lane.h)    order2 and wide_advance, unchanged; fetch_wide_or_triangle's shape and row loads,
//               here over five descriptors (fetch_two_level_wide)
// Per iteration a lane holds one of four kinds: a wide node of either level (seven rows: row 7, the child count, is for the host), a
// triangle (four rows), an entering link (the record's four rows plus the mask word) or a marker (nothing).  The loads of one iteration
// sit under exec masks with a single wait, a kind that no lane holds is skipped by a scalar branch, and every fetch goes through a
// wave-uniform range-checked descriptor: whatever a link, an offset or a record holds, a lane reads zeros and never faults.  Inside an
// instance a wide node is fetched only below the record's extent, so an instance of extent 0 reads nothing.
// Arithmetic is the GENERIC path only, as in the binary two-level trace (an opt-in sibling votes per wave and iteration between GENERIC
// and FAST: trace_instanced_wide_fast_kernels.hip, NTR_TIW_FAST).  The loop is stated once (trace_instanced_wide_body.h; its
// parameters and fetch are in trace_instanced_wide_kernels.h) and instantiated three ways here:
//   trace_instanced_wide<false, false>   unmasked: vis == NULL, or a vis that can refuse nothing
//   trace_instanced_wide<true, false>    visibility masks
//   trace_instanced_wide<true, true>     the masked loop with per-lane counters (ntr_trace_instanced_wide_stats; not a timed path)
// and twice more, seeded, in trace_instanced_wide_seeded_kernels.hip (ntr_trace_instanced_wide_seeded and its _stats form, whose entry
// points are here; the rule is tests/np_instanced_seeded.py).  Of the host side the unit holds the fill of the kernels'
// parameters, the choice among the five and their entry points; the launch around them is trace_instanced_launch.h's, shared with the
// three sibling units.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "instanced_wide_bvh.h"
#include "trace_instanced_launch.h"
#include "trace_lane.h"
#include "trace_wide_lane.h"
#include "trace_instanced_wide_kernels.h"

namespace ntr {
namespace {

#define NTR_TIW_TEMPLATE template <bool MASKED, bool STATS>
#define NTR_TIW_KERNEL trace_instanced_wide
#define NTR_TIW_PARAMS InstancedWideParams p
#define NTR_TIW_SEEDED 0
#define NTR_TIW_FAST 0
#include "trace_instanced_wide_body.h"
#undef NTR_TIW_TEMPLATE
#undef NTR_TIW_KERNEL
#undef NTR_TIW_PARAMS
#undef NTR_TIW_SEEDED
#undef NTR_TIW_FAST

// The unit's launch under the shared path (trace_instanced_launch.h).  vis == NULL, or a vis that can refuse nothing (no arrays and
// rayMask all ones), launches the unmasked kernel; stats != NULL launches an instrumented one; a seed the seeded kernels of
// trace_instanced_wide_seeded_kernels.hip (always the masked loop).
int trace_instanced_wide_call(const TwoLevelCall& c)
{
    return two_level_trace(c, [&c](DeviceState* ds, hipStream_t s, unsigned int blocks) {
        InstancedWideParams p{};
        two_level_fill(p, c, ds);
        p.poolWide = c.poolNodes; p.poolWideBytes = (uint32_t)c.poolNodesBytes;
        const bool masked = two_level_fill_visibility(p, c, ds);
        const dim3 grid(blocks), block(64);
        if (c.seed == TwoLevelSeed::kRequired) {
            InstancedWideSeed sd{};
            sd.seedResults = c.seedResults; sd.seedInstance = c.seedInstance;
            launch_trace_instanced_wide_seeded(c.stats != nullptr, blocks, s, &p, &sd);
        } else if (c.stats) {
            hipLaunchKernelGGL((trace_instanced_wide<true, true>), grid, block, 0, s, p);
        } else if (masked) {
            hipLaunchKernelGGL((trace_instanced_wide<true, false>), grid, block, 0, s, p);
        } else {
            hipLaunchKernelGGL((trace_instanced_wide<false, false>), grid, block, 0, s, p);
        }
    });
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" int ntr_trace_instanced_wide(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                        const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink, const void* d_wideRecords,
                                        int32_t numInstances, const void* d_widePoolNodes, int64_t widePoolNodesBytes,
                                        const void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                        const NtrInstanceVisibility* vis, float* seconds, void* stream)
{
    return trace_instanced_wide_call({"ntr_trace_instanced_wide", kTwoLevelWide, TwoLevelSeed::kNone, nullptr, numRays, anyHit, d_rays, nullptr, -1,
                                      d_results, d_instanceIDs, d_wideTlasNodes, wideTlasNodesBytes, rootLink, d_wideRecords, numInstances,
                                      d_widePoolNodes, widePoolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, nullptr, seconds,
                                      stream, nullptr, nullptr});
}

extern "C" int ntr_trace_instanced_wide_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                                              int32_t* d_instanceIDs, const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                                              const void* d_wideRecords, int32_t numInstances, const void* d_widePoolNodes,
                                              int64_t widePoolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                              const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis, NtrInstancedTraceStats* stats,
                                              void* stream)
{
    if (!stats) return set_error(NTR_ERR_INVALID, "ntr_trace_instanced_wide_stats: null stats");
    return trace_instanced_wide_call({"ntr_trace_instanced_wide_stats", kTwoLevelWide, TwoLevelSeed::kNone, nullptr, numRays, anyHit, d_rays, nullptr,
                                      -1, d_results, d_instanceIDs, d_wideTlasNodes, wideTlasNodesBytes, rootLink, d_wideRecords, numInstances,
                                      d_widePoolNodes, widePoolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, nullptr, nullptr,
                                      stream, stats, nullptr});
}

extern "C" int ntr_trace_instanced_wide_seeded(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                               int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                               const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                                               const void* d_wideRecords, int32_t numInstances, const void* d_widePoolNodes,
                                               int64_t widePoolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                               const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis, float* seconds, void* stream)
{
    return trace_instanced_wide_call({"ntr_trace_instanced_wide_seeded", kTwoLevelWide, TwoLevelSeed::kRequired, nullptr, numRays, anyHit, d_rays,
                                      d_seedResults, seedInstance, d_results, d_instanceIDs, d_wideTlasNodes, wideTlasNodesBytes, rootLink,
                                      d_wideRecords, numInstances, d_widePoolNodes, widePoolNodesBytes, d_poolTriWoop, poolTriWoopBytes,
                                      d_poolTriIndex, vis, nullptr, seconds, stream, nullptr, nullptr});
}

extern "C" int ntr_trace_instanced_wide_seeded_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                                     int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                                     const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                                                     const void* d_wideRecords, int32_t numInstances, const void* d_widePoolNodes,
                                                     int64_t widePoolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                                     const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis,
                                                     NtrInstancedTraceStats* stats, void* stream)
{
    if (!stats) return set_error(NTR_ERR_INVALID, "ntr_trace_instanced_wide_seeded_stats: null stats");
    return trace_instanced_wide_call({"ntr_trace_instanced_wide_seeded_stats", kTwoLevelWide, TwoLevelSeed::kRequired, nullptr, numRays, anyHit,
                                      d_rays, d_seedResults, seedInstance, d_results, d_instanceIDs, d_wideTlasNodes, wideTlasNodesBytes, rootLink,
                                      d_wideRecords, numInstances, d_widePoolNodes, widePoolNodesBytes, d_poolTriWoop, poolTriWoopBytes,
                                      d_poolTriIndex, vis, nullptr, nullptr, stream, stats, nullptr});
}
