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
// points are here; the rule is tests/np_instanced_seeded.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "instanced_wide_bvh.h"
#include "device_scratch.h"
#include "sched_state.h"
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

// The entry points' one body.  vis == NULL, or a vis that can refuse nothing (no arrays and rayMask all ones), launches the unmasked
// kernel; stats != NULL launches the instrumented one and reads the counters back.  seeded: the seeded kernels of
// trace_instanced_wide_seeded_kernels.hip (always the masked loop).
int trace_instanced_wide_impl(const char* fn, int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                              int32_t* d_instanceIDs, const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                              const void* d_wideRecords, int32_t numInstances, const void* d_widePoolNodes, int64_t widePoolNodesBytes,
                              const void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                              const NtrInstanceVisibility* vis, float* seconds, void* stream, NtrInstancedTraceStats* stats,
                              bool seeded = false, const NtrRayResult* d_seedResults = nullptr, int32_t seedInstance = -1)
{
    if (seconds) *seconds = 0.0f;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (numRays < 0) return set_error(NTR_ERR_INVALID, "%s: numRays < 0", fn);
    if (numRays == 0) return NTR_OK;
    if (!d_rays || !d_results || !d_instanceIDs) return set_error(NTR_ERR_INVALID, "%s: null ray, result or instance id buffer", fn);
    if (numInstances < 1 || (int64_t)numInstances * kRecordBytes > kPoolMaxBytes || !d_wideRecords || !d_widePoolNodes || !d_poolTriWoop ||
        !d_poolTriIndex)
        return set_error(NTR_ERR_INVALID, "%s: no instances or no pool", fn);
    if (!(rootLink == 0 || (rootLink < 0 && (int64_t)~rootLink < numInstances)))
        return set_error(NTR_ERR_INVALID, "%s: rootLink %d is neither 0 nor an instance's link", fn, (int)rootLink);
    if (wideTlasNodesBytes < 0 || (wideTlasNodesBytes % kWideBytes) != 0 || wideTlasNodesBytes > kMaxWideBytes ||
        (rootLink == 0 && (!d_wideTlasNodes || wideTlasNodesBytes < kWideBytes)))
        return set_error(NTR_ERR_INVALID, "%s: the wide top-level node buffer must be a multiple of 128 bytes, at most 0x%llx, and hold the root",
                         fn, (unsigned long long)kMaxWideBytes);
    if (const int rc = check_wide_pool_bytes(fn, "widePoolNodesBytes", widePoolNodesBytes)) return rc;
    if (const int rc = check_pool_bytes(fn, "poolTriWoopBytes", poolTriWoopBytes, kRowBytes)) return rc;
    if (vis && ((((uintptr_t)vis->d_instanceMasks) | ((uintptr_t)vis->d_rayMasks)) & 3u) != 0)
        return set_error(NTR_ERR_INVALID, "%s: a mask array must be 4-byte aligned", fn);
    if (seeded && (!d_seedResults || (((uintptr_t)d_seedResults) & 15u) != 0))
        return set_error(NTR_ERR_INVALID, "%s: the seed records must be given and 16-byte aligned", fn);

    DeviceState* ds = nullptr;
    if (const int rc = current_device_state_ready(&ds)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (stats && stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "%s: the call reads its counters back and cannot be captured", fn);
    InstancedWideParams p{};
    p.numRays = numRays; p.anyHit = anyHit ? 1 : 0; p.rays = d_rays; p.results = d_results; p.instanceIDs = d_instanceIDs;
    p.tlas = d_wideTlasNodes; p.records = d_wideRecords; p.poolWide = d_widePoolNodes; p.poolWoop = d_poolTriWoop;
    p.tlasBytes = d_wideTlasNodes ? (uint32_t)wideTlasNodesBytes : 0u; p.recordsBytes = (uint32_t)((int64_t)numInstances * kRecordBytes);
    p.poolWideBytes = (uint32_t)widePoolNodesBytes; p.poolWoopBytes = (uint32_t)poolTriWoopBytes;
    p.triIndex = d_poolTriIndex; p.rootLink = rootLink; p.numInstances = numInstances; p.status = ds->status;
    p.rayMask = 0xFFFFFFFFu;
    if (vis) {
        p.instMasks = vis->d_instanceMasks; p.instMasksBytes = vis->d_instanceMasks ? (uint32_t)((int64_t)numInstances * 4) : 0u;
        p.rayMasks = vis->d_rayMasks; p.rayMask = vis->rayMask;
    }
    p.stats = ds->stats;
    const bool masked = p.instMasks || p.rayMasks || p.rayMask != 0xFFFFFFFFu;

    StreamEvents<2> ev(s);   // the timed bracket
    if (seconds) {
        NTR_HIP(ev.create());
        NTR_HIP(hipStreamSynchronize(s));
        NTR_HIP(ev.record(0));
    }
    const dim3 grid((numRays + 63) / 64), block(64);
    if (stats) NTR_HIP(hipMemsetAsync(ds->stats, 0, 7 * sizeof(unsigned long long), s));
    if (seeded) {
        InstancedWideSeed sd{};
        sd.seedResults = d_seedResults; sd.seedInstance = seedInstance;
        launch_trace_instanced_wide_seeded(stats != nullptr, grid.x, s, &p, &sd);
    } else if (stats) {
        hipLaunchKernelGGL((trace_instanced_wide<true, true>), grid, block, 0, s, p);
    } else if (masked) {
        hipLaunchKernelGGL((trace_instanced_wide<true, false>), grid, block, 0, s, p);
    } else {
        hipLaunchKernelGGL((trace_instanced_wide<false, false>), grid, block, 0, s, p);
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

extern "C" int ntr_trace_instanced_wide(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                        const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink, const void* d_wideRecords,
                                        int32_t numInstances, const void* d_widePoolNodes, int64_t widePoolNodesBytes,
                                        const void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                        const NtrInstanceVisibility* vis, float* seconds, void* stream)
{
    return trace_instanced_wide_impl("ntr_trace_instanced_wide", numRays, anyHit, d_rays, d_results, d_instanceIDs, d_wideTlasNodes,
                                     wideTlasNodesBytes, rootLink, d_wideRecords, numInstances, d_widePoolNodes, widePoolNodesBytes,
                                     d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, seconds, stream, nullptr);
}

extern "C" int ntr_trace_instanced_wide_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                                              int32_t* d_instanceIDs, const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                                              const void* d_wideRecords, int32_t numInstances, const void* d_widePoolNodes,
                                              int64_t widePoolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                              const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis, NtrInstancedTraceStats* stats,
                                              void* stream)
{
    if (!stats) return set_error(NTR_ERR_INVALID, "ntr_trace_instanced_wide_stats: null stats");
    return trace_instanced_wide_impl("ntr_trace_instanced_wide_stats", numRays, anyHit, d_rays, d_results, d_instanceIDs, d_wideTlasNodes,
                                     wideTlasNodesBytes, rootLink, d_wideRecords, numInstances, d_widePoolNodes, widePoolNodesBytes,
                                     d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, nullptr, stream, stats);
}

extern "C" int ntr_trace_instanced_wide_seeded(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, const NtrRayResult* d_seedResults,
                                               int32_t seedInstance, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                               const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                                               const void* d_wideRecords, int32_t numInstances, const void* d_widePoolNodes,
                                               int64_t widePoolNodesBytes, const void* d_poolTriWoop, int64_t poolTriWoopBytes,
                                               const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis, float* seconds, void* stream)
{
    return trace_instanced_wide_impl("ntr_trace_instanced_wide_seeded", numRays, anyHit, d_rays, d_results, d_instanceIDs, d_wideTlasNodes,
                                     wideTlasNodesBytes, rootLink, d_wideRecords, numInstances, d_widePoolNodes, widePoolNodesBytes,
                                     d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, seconds, stream, nullptr, true, d_seedResults,
                                     seedInstance);
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
    return trace_instanced_wide_impl("ntr_trace_instanced_wide_seeded_stats", numRays, anyHit, d_rays, d_results, d_instanceIDs,
                                     d_wideTlasNodes, wideTlasNodesBytes, rootLink, d_wideRecords, numInstances, d_widePoolNodes,
                                     widePoolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, nullptr, stream, stats, true,
                                     d_seedResults, seedInstance);
}
