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
// Four kernels: trace_instanced_fast, trace_instanced_fast_seeded and their instrumented variants.  The entry points are here too, not
// in trace_instanced_kernels.hip: that unit stays as it was (trace_instanced_kernels.h: why).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "instanced_bvh.h"
#include "device_scratch.h"
#include "sched_state.h"
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

// The two entry points' one body: trace_instanced_impl's checks (trace_instanced_kernels.hip) and d_flags; stats != NULL launches an
// instrumented kernel and reads the eleven counters back.
int trace_instanced_fast_impl(const char* fn, int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                              int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs, const void* d_tlasNodes,
                              int64_t tlasNodesBytes, int32_t rootLink, const void* d_records, int32_t numInstances, const void* d_poolNodes,
                              int64_t poolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                              const NtrInstanceVisibility* vis, const uint32_t* d_flags, float* seconds, void* stream,
                              NtrInstancedTraceStats* stats, NtrInstancedFastStats* fastStats)
{
    if (seconds) *seconds = 0.0f;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (fastStats) memset(fastStats, 0, sizeof(*fastStats));
    if ((stats != nullptr) != (fastStats != nullptr)) return set_error(NTR_ERR_INVALID, "%s: null stats", fn);
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
    if ((((uintptr_t)d_seedResults) & 15u) != 0) return set_error(NTR_ERR_INVALID, "%s: the seed records must be 16-byte aligned", fn);
    if (!d_flags || (((uintptr_t)d_flags) & 15u) != 0)
        return set_error(NTR_ERR_INVALID, "%s: the flags (ntr_instanced_validate) must be given and 16-byte aligned", fn);

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
    x.stats = ds->stats;   // STATS: InstancedExtras's seven, and at [8..11] {wave steps, FAST wave steps, nice starts, nice entries} (of 32 words)
    InstancedFast f{};
    f.flags = d_flags;
    InstancedSeed sd{};
    sd.seedResults = d_seedResults; sd.seedInstance = seedInstance;

    StreamEvents<2> ev(s);   // the timed bracket
    if (seconds) {
        NTR_HIP(ev.create());
        NTR_HIP(hipStreamSynchronize(s));
        NTR_HIP(ev.record(0));
    }
    const dim3 grid((numRays + 63) / 64), block(64);
    if (stats) NTR_HIP(hipMemsetAsync(ds->stats, 0, 12 * sizeof(unsigned long long), s));
    if (d_seedResults) {
        if (stats) hipLaunchKernelGGL(trace_instanced_fast_seeded_stats, grid, block, 0, s, p, x, sd, f);
        else hipLaunchKernelGGL(trace_instanced_fast_seeded, grid, block, 0, s, p, x, sd, f);
    } else {
        if (stats) hipLaunchKernelGGL(trace_instanced_fast_stats, grid, block, 0, s, p, x, f);
        else hipLaunchKernelGGL(trace_instanced_fast, grid, block, 0, s, p, x, f);
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
        unsigned long long h[12];
        NTR_HIP(hipMemcpyAsync(h, ds->stats, sizeof(h), hipMemcpyDeviceToHost, s));
        NTR_HIP(hipStreamSynchronize(s));
        stats->numRays = numRays;
        stats->numTopInnerVisits = (int64_t)h[0]; stats->numInstanceEntries = (int64_t)h[1]; stats->numInstancesMasked = (int64_t)h[2];
        stats->numInnerVisits = (int64_t)h[3]; stats->numTriTests = (int64_t)h[4]; stats->numLeafVisits = (int64_t)h[5];
        stats->numHits = (int64_t)h[6];
        fastStats->waveSteps = h[8]; fastStats->fastWaveSteps = h[9]; fastStats->niceStarts = h[10]; fastStats->niceEntries = h[11];
    }
    return NTR_OK;
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
    return trace_instanced_fast_impl("ntr_trace_instanced_fast", numRays, anyHit, d_rays, d_seedResults, seedInstance, d_results, d_instanceIDs,
                                     d_tlasNodes, tlasNodesBytes, rootLink, d_records, numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop,
                                     poolTriWoopBytes, d_poolTriIndex, vis, d_flags, seconds, stream, nullptr, nullptr);
}

extern "C" int ntr_trace_instanced_fast_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                              int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs, const void* d_tlasNodes,
                                              int64_t tlasNodesBytes, int32_t rootLink, const void* d_records, int32_t numInstances,
                                              const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                              int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis,
                                              const uint32_t* d_flags, NtrInstancedTraceStats* stats, NtrInstancedFastStats* fastStats,
                                              void* stream)
{
    if (stats) memset(stats, 0, sizeof(*stats));
    if (fastStats) memset(fastStats, 0, sizeof(*fastStats));
    if (!stats || !fastStats) return set_error(NTR_ERR_INVALID, "ntr_trace_instanced_fast_stats: null stats");
    return trace_instanced_fast_impl("ntr_trace_instanced_fast_stats", numRays, anyHit, d_rays, d_seedResults, seedInstance, d_results,
                                     d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records, numInstances, d_poolNodes, poolNodesBytes,
                                     d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, d_flags, nullptr, stream, stats, fastStats);
}
