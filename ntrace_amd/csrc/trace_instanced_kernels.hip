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
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "instanced_bvh.h"
#include "device_scratch.h"
#include "sched_state.h"
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

// The entry points' one body.  vis == NULL, or a vis that can refuse nothing (no arrays and rayMask all ones), launches the unmasked
// kernel; stats != NULL launches the instrumented one and reads the counters back.  seeded: the seeded kernels (always the masked loop).
int trace_instanced_impl(const char* fn, int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                         const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records, int32_t numInstances,
                         const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                         const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis, float* seconds, void* stream,
                         NtrInstancedTraceStats* stats, bool seeded = false, const NtrRayResult* d_seedResults = nullptr, int32_t seedInstance = -1)
{
    if (seconds) *seconds = 0.0f;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (numRays < 0) return set_error(NTR_ERR_INVALID, "%s: numRays < 0", fn);
    if (numRays == 0) return NTR_OK;
    if (!d_rays || !d_results || !d_instanceIDs) return set_error(NTR_ERR_INVALID, "%s: null ray, result or instance id buffer", fn);
    if (numInstances < 1 || (int64_t)numInstances * kRecordBytes > kPoolMaxBytes || !d_records || !d_poolNodes || !d_poolTriWoop || !d_poolTriIndex)
        return set_error(NTR_ERR_INVALID, "%s: no instances or no pool", fn);
    if (!(rootLink == 0 || (rootLink < 0 && (int64_t)~rootLink < numInstances)))
        return set_error(NTR_ERR_INVALID, "%s: rootLink %d is neither 0 nor an instance's link", fn, (int)rootLink);
    if (tlasNodesBytes < 0 || (tlasNodesBytes % kNodeBytes) != 0 || tlasNodesBytes > kMaxNodesBytes || (rootLink == 0 && (!d_tlasNodes || tlasNodesBytes < kNodeBytes)))
        return set_error(NTR_ERR_INVALID, "%s: the top-level node buffer must be a multiple of 64 bytes, at most 0x%llx, and hold the root", fn,
                         (unsigned long long)kMaxNodesBytes);
    if (const int rc = check_pool_bytes(fn, "poolNodesBytes", poolNodesBytes, kNodeBytes)) return rc;
    if (const int rc = check_pool_bytes(fn, "poolTriWoopBytes", poolTriWoopBytes, kRowBytes)) return rc;
    if (vis && ((((uintptr_t)vis->d_instanceMasks) | ((uintptr_t)vis->d_rayMasks)) & 3u) != 0)
        return set_error(NTR_ERR_INVALID, "%s: a mask array must be 4-byte aligned", fn);
    if (seeded && (!d_seedResults || (((uintptr_t)d_seedResults) & 15u) != 0))
        return set_error(NTR_ERR_INVALID, "%s: the seed records must be given and 16-byte aligned", fn);

    DeviceState* ds = nullptr;
    if (const int rc = current_device_state_ready(&ds)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (stats && stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "%s: the call reads its counters back and cannot be captured", fn);
    InstancedParams p{};
    p.numRays = numRays; p.anyHit = anyHit ? 1 : 0; p.rays = d_rays; p.results = d_results; p.instanceIDs = d_instanceIDs;
    p.tlas = d_tlasNodes; p.records = d_records; p.poolNodes = d_poolNodes; p.poolWoop = d_poolTriWoop;
    p.tlasBytes = d_tlasNodes ? (uint32_t)tlasNodesBytes : 0u; p.recordsBytes = (uint32_t)((int64_t)numInstances * kRecordBytes);
    p.poolNodesBytes = (uint32_t)poolNodesBytes; p.poolWoopBytes = (uint32_t)poolTriWoopBytes;
    p.triIndex = d_poolTriIndex; p.rootLink = rootLink; p.numInstances = numInstances; p.status = ds->status;
    InstancedExtras x{};
    x.rayMask = 0xFFFFFFFFu;
    if (vis) {
        x.instMasks = vis->d_instanceMasks; x.instMasksBytes = vis->d_instanceMasks ? (uint32_t)((int64_t)numInstances * 4) : 0u;
        x.rayMasks = vis->d_rayMasks; x.rayMask = vis->rayMask;
    }
    x.stats = ds->stats;
    const bool masked = x.instMasks || x.rayMasks || x.rayMask != 0xFFFFFFFFu;

    StreamEvents<2> ev(s);   // the timed bracket
    if (seconds) {
        NTR_HIP(ev.create());
        NTR_HIP(hipStreamSynchronize(s));
        NTR_HIP(ev.record(0));
    }
    const dim3 grid((numRays + 63) / 64), block(64);
    if (stats) NTR_HIP(hipMemsetAsync(ds->stats, 0, 7 * sizeof(unsigned long long), s));
    if (seeded) {
        InstancedSeed sd{};
        sd.seedResults = d_seedResults; sd.seedInstance = seedInstance;
        launch_trace_instanced_seeded(stats != nullptr, grid.x, s, &p, &x, &sd);
    } else if (stats) {
        launch_trace_instanced_variant(true, grid.x, s, &p, &x);
    } else if (masked) {
        launch_trace_instanced_variant(false, grid.x, s, &p, &x);
    } else {
        hipLaunchKernelGGL(trace_instanced, grid, block, 0, s, p);
    }
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
    if (stats) {
        unsigned long long h[7];
        NTR_HIP(hipMemcpyAsync(h, ds->stats, sizeof(h), hipMemcpyDeviceToHost, s));
        NTR_HIP(hipStreamSynchronize(s));
        stats->numRays = numRays;
        stats->numTopInnerVisits = (int64_t)h[0]; stats->numInstanceEntries = (int64_t)h[1]; stats->numInstancesMasked = (int64_t)h[2];
        stats->numInnerVisits = (int64_t)h[3]; stats->numTriTests = (int64_t)h[4]; stats->numLeafVisits = (int64_t)h[5];
        stats->numHits = (int64_t)h[6];
    }
    return NTR_OK;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" int ntr_trace_instanced(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                   const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                   int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                   int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, float* seconds, void* stream)
{
    return trace_instanced_impl("ntr_trace_instanced", numRays, anyHit, d_rays, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink,
                                d_records, numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, nullptr,
                                seconds, stream, nullptr);
}

extern "C" int ntr_trace_instanced_masked(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                          const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                          int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                          int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis,
                                          float* seconds, void* stream)
{
    return trace_instanced_impl("ntr_trace_instanced_masked", numRays, anyHit, d_rays, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes,
                                rootLink, d_records, numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex,
                                vis, seconds, stream, nullptr);
}

extern "C" int ntr_trace_instanced_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                         const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                         int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                         int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis,
                                         NtrInstancedTraceStats* stats, void* stream)
{
    if (!stats) return set_error(NTR_ERR_INVALID, "ntr_trace_instanced_stats: null stats");
    return trace_instanced_impl("ntr_trace_instanced_stats", numRays, anyHit, d_rays, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes,
                                rootLink, d_records, numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex,
                                vis, nullptr, stream, stats);
}

extern "C" int ntr_trace_instanced_seeded(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                          int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs, const void* d_tlasNodes,
                                          int64_t tlasNodesBytes, int32_t rootLink, const void* d_records, int32_t numInstances,
                                          const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                          const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis, float* seconds, void* stream)
{
    return trace_instanced_impl("ntr_trace_instanced_seeded", numRays, anyHit, d_rays, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes,
                                rootLink, d_records, numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex,
                                vis, seconds, stream, nullptr, true, d_seedResults, seedInstance);
}

extern "C" int ntr_trace_instanced_seeded_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                                int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs, const void* d_tlasNodes,
                                                int64_t tlasNodesBytes, int32_t rootLink, const void* d_records, int32_t numInstances,
                                                const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                                int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis,
                                                NtrInstancedTraceStats* stats, void* stream)
{
    if (!stats) return set_error(NTR_ERR_INVALID, "ntr_trace_instanced_seeded_stats: null stats");
    return trace_instanced_impl("ntr_trace_instanced_seeded_stats", numRays, anyHit, d_rays, d_results, d_instanceIDs, d_tlasNodes,
                                tlasNodesBytes, rootLink, d_records, numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes,
                                d_poolTriIndex, vis, nullptr, stream, stats, true, d_seedResults, seedInstance);
}
