// trace_instanced_kernels.hip -- the two-level trace for gfx950 (ntr_trace_instanced): a top-level tree over instances, each a Compact
// tree of a pool plus a transform (instanced_bvh.h).  EXTENSION: the reference has no instancing; the rule is the numpy spec
// tests/np_instanced.py, which the kernel equals in all four result words and the instance id.
// One kernel, 64-thread workgroups, one ray per lane: a unified-step loop built from trace_lane.h.  Per iteration every live lane fetches
// the 64 bytes it needs -- a top-level node, an instance record, a BLAS node at nodesOffset + node, or a triangle and the word after it
// at row offset + row -- and takes the step they allow:
//   inner node (either level)   inner_advance<false, 8>, unchanged
//   triangle                    triangle_step, through unified_advance, unchanged
//   entering an instance        (top level, link ~i) push the exit marker, transform the ray by record i, go on at the BLAS's node 0
//   leaving an instance         (the exit marker was popped) reload the world ray from d_rays -- one 32-byte load, rare against the
//                               steps, for six registers less -- and pop again
// Arithmetic is the GENERIC path only: a transformed ray need not lie in the FAST ranges, and the pool has no validate flags.  (Both
// are answered by an opt-in sibling, not here: trace_instanced_fast_kernels.hip, NTR_TI_FAST)
// Fetches go through four wave-uniform range-checked descriptors (fetch64_four_buffers: the shape of fetch64_two_buffers): whatever a
// link or an offset holds, a lane reads zeros and never faults.  Per lane beyond the single-level loop: nodesOffset, the row offset
// and the instance index, which also says which level the lane is on (-1: the top level).
// The loop is stated once (trace_instanced_body.h) and instantiated three ways (the rule is tests/np_instanced_masked.py),
// the first here and the other two in trace_instanced_masked_kernels.hip (trace_instanced_kernels.h: why two units):
//   trace_instanced          unmasked: ntr_trace_instanced, and ntr_trace_instanced_masked when no mask can refuse anything
//   trace_instanced_masked   visibility: the ray's mask m_r is loaded once beside the ray; a lane that enters instance i reads M_i through a
//                            fifth descriptor over 4 * numInstances bytes, in the same fetch and the same wait as the record, and pops when
//                            (M_i & m_r) == 0 -- no marker, no transform, the record dropped.  Without instance masks the group of that
//                            load has an empty mask and is skipped by its scalar branch
//   trace_instanced_stats    the masked loop with per-lane counters, added once at the end (ntr_trace_instanced_stats; not a timed path)
// and twice more, seeded (NTR_TI_SEEDED; trace_instanced_seeded_kernels.hip; the rule is tests/np_instanced_seeded.py):
//   trace_instanced_seeded, trace_instanced_seeded_stats   the masked and the instrumented loop started from one result record per ray
// Of the host side the unit holds the fill of the kernels' parameters, the choice among the five and their entry points; the launch
// around them is trace_instanced_launch.h's, shared with the three sibling units.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "instanced_bvh.h"
#include "trace_instanced_launch.h"
#include "trace_lane.h"
#include "trace_instanced_kernels.h"

namespace ntr {
namespace {

#define NTR_TI_KERNEL trace_instanced
#define NTR_TI_PARAMS InstancedParams p
#define NTR_TI_MASKED 0
#define NTR_TI_STATS 0
#define NTR_TI_SEEDED 0
#define NTR_TI_FAST 0
#include "trace_instanced_body.h"
#undef NTR_TI_KERNEL
#undef NTR_TI_PARAMS
#undef NTR_TI_MASKED
#undef NTR_TI_STATS
#undef NTR_TI_SEEDED
#undef NTR_TI_FAST

// The unit's launch under the shared path (trace_instanced_launch.h).  vis == NULL, or a vis that can refuse nothing (no arrays and
// rayMask all ones), launches the unmasked kernel; stats != NULL launches an instrumented one; a seed the seeded kernels (always the
// masked loop).
int trace_instanced_call(const TwoLevelCall& c)
{
    return two_level_trace(c, [&c](DeviceState* ds, hipStream_t s, unsigned int blocks) {
        InstancedParams p{};
        two_level_fill(p, c, ds);
        p.poolNodes = c.poolNodes; p.poolNodesBytes = (uint32_t)c.poolNodesBytes;
        InstancedExtras x{};
        const bool masked = two_level_fill_visibility(x, c, ds);
        if (c.seed == TwoLevelSeed::kRequired) {
            InstancedSeed sd{};
            sd.seedResults = c.seedResults; sd.seedInstance = c.seedInstance;
            launch_trace_instanced_seeded(c.stats != nullptr, blocks, s, &p, &x, &sd);
        } else if (c.stats || masked) {
            launch_trace_instanced_variant(c.stats != nullptr, blocks, s, &p, &x);
        } else {
            hipLaunchKernelGGL(trace_instanced, dim3(blocks), dim3(64), 0, s, p);
        }
    });
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" int ntr_trace_instanced(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                   const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                   int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                   int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, float* seconds, void* stream)
{
    return trace_instanced_call({"ntr_trace_instanced", kTwoLevelBinary, TwoLevelSeed::kNone, nullptr, numRays, anyHit, d_rays, nullptr, -1,
                                 d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records, numInstances, d_poolNodes,
                                 poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, nullptr, nullptr, seconds, stream, nullptr,
                                 nullptr});
}

extern "C" int ntr_trace_instanced_masked(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                          const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                          int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                          int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis,
                                          float* seconds, void* stream)
{
    return trace_instanced_call({"ntr_trace_instanced_masked", kTwoLevelBinary, TwoLevelSeed::kNone, nullptr, numRays, anyHit, d_rays, nullptr, -1,
                                 d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records, numInstances, d_poolNodes,
                                 poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, nullptr, seconds, stream, nullptr,
                                 nullptr});
}

extern "C" int ntr_trace_instanced_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                         const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                         int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                         int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis,
                                         NtrInstancedTraceStats* stats, void* stream)
{
    if (!stats) return set_error(NTR_ERR_INVALID, "ntr_trace_instanced_stats: null stats");
    return trace_instanced_call({"ntr_trace_instanced_stats", kTwoLevelBinary, TwoLevelSeed::kNone, nullptr, numRays, anyHit, d_rays, nullptr, -1,
                                 d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records, numInstances, d_poolNodes,
                                 poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, nullptr, nullptr, stream, stats, nullptr});
}

extern "C" int ntr_trace_instanced_seeded(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                          int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs, const void* d_tlasNodes,
                                          int64_t tlasNodesBytes, int32_t rootLink, const void* d_records, int32_t numInstances,
                                          const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                          const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis, float* seconds, void* stream)
{
    return trace_instanced_call({"ntr_trace_instanced_seeded", kTwoLevelBinary, TwoLevelSeed::kRequired, nullptr, numRays, anyHit, d_rays,
                                 d_seedResults, seedInstance, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records,
                                 numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, nullptr, seconds,
                                 stream, nullptr, nullptr});
}

extern "C" int ntr_trace_instanced_seeded_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                                int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs, const void* d_tlasNodes,
                                                int64_t tlasNodesBytes, int32_t rootLink, const void* d_records, int32_t numInstances,
                                                const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                                int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis,
                                                NtrInstancedTraceStats* stats, void* stream)
{
    if (!stats) return set_error(NTR_ERR_INVALID, "ntr_trace_instanced_seeded_stats: null stats");
    return trace_instanced_call({"ntr_trace_instanced_seeded_stats", kTwoLevelBinary, TwoLevelSeed::kRequired, nullptr, numRays, anyHit, d_rays,
                                 d_seedResults, seedInstance, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records,
                                 numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, nullptr, nullptr,
                                 stream, stats, nullptr});
}
