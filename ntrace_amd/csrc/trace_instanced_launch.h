// trace_instanced_launch.h -- host only: the launch of the two-level trace, stated once for its seven units:
//   trace_instanced_kernels.hip            ntr_trace_instanced, _masked, _stats, _seeded, _seeded_stats
//   trace_instanced_fast_kernels.hip       ntr_trace_instanced_fast, _fast_stats
//   trace_instanced_wide_kernels.hip       ntr_trace_instanced_wide, _wide_stats, _wide_seeded, _wide_seeded_stats
//   trace_instanced_wide_fast_kernels.hip  ntr_trace_instanced_wide_fast, _wide_fast_stats
//   trace_instanced_motion_kernels.hip     ntr_trace_instanced_motion, _motion_stats
//   trace_instanced_wide_motion_kernels.hip  ntr_trace_instanced_wide_motion, _wide_motion_stats
//   trace_instanced_deform_kernels.hip     ntr_trace_instanced_deform, _deform_stats
// An entry point writes what it was given into a TwoLevelCall, with the few facts in which the units differ, and calls two_level_trace
// with its unit's launch: the checks, the device state, the bracket (trace_launch.h) and the counters' unpacking are here; the kernels,
// the fill of their parameters and the choice among them stay with the unit (trace_instanced_kernels.h: why the units are separate).
// What the checks refuse, in which words and in which order, is pinned by tests/test_two_level_refusals_cpu.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "instance_motion.h"
#include "instanced_wide_bvh.h"
#include "trace_launch.h"

namespace ntr {

// The two layouts: the unit and the cap of the top-level node buffer and of a BLAS in the pool, and the words of their refusals
struct TwoLevelLayout {
    int unit;
    int64_t tlasMaxBytes;
    const char *tlasRefusal, *poolNodesName;
};
constexpr TwoLevelLayout kTwoLevelBinary = {kNodeBytes, kMaxNodesBytes,
                                            "%s: the top-level node buffer must be a multiple of 64 bytes, at most 0x%llx, and hold the root",
                                            "poolNodesBytes"};
constexpr TwoLevelLayout kTwoLevelWide = {kWideBytes, kMaxWideBytes,
                                          "%s: the wide top-level node buffer must be a multiple of 128 bytes, at most 0x%llx, and hold the root",
                                          "widePoolNodesBytes"};
enum class TwoLevelSeed { kNone, kRequired, kOptional };

// What an entry point was given, in the order of the widest parameter list (an entry point without an argument passes NULL, and -1 for
// seedInstance), after the three facts about the entry point itself.
struct TwoLevelCall {
    const char* fn;
    const TwoLevelLayout& layout;
    TwoLevelSeed seed;
    const char* validate;   // the FAST units: d_flags must be given, and this call writes them; NULL: no flags
    int32_t numRays, anyHit;
    const NtrRay* rays;
    const NtrRayResult* seedResults;
    int32_t seedInstance;
    NtrRayResult* results;
    int32_t* instanceIDs;
    const void* tlas;
    int64_t tlasBytes;
    int32_t rootLink;
    const void* records;
    int32_t numInstances;
    const void* poolNodes;
    int64_t poolNodesBytes;
    const void* poolTriWoop;
    int64_t poolTriWoopBytes;
    const int32_t* poolTriIndex;
    const NtrInstanceVisibility* vis;
    const uint32_t* d_flags;
    float* seconds;
    void* stream;
    NtrInstancedTraceStats* stats;      // both NULL, or the instrumented kernel; a FAST unit takes both or neither
    NtrInstancedFastStats* fastStats;
    const NtrInstanceMotion* motion;    // the two motion units: given; every other unit leaves the two NULL
    NtrInstancedMotionStats* motionStats;   // with stats, or NULL
    // trailing and defaulted: the aggregate initialisers of the units that came before stay as they are
    const NtrInstanceDeform* deform = nullptr;        // the deform unit: given; it needs `motion`
    NtrInstancedDeformStats* deformStats = nullptr;   // with stats, or NULL
};

// What a call that takes an NtrInstanceDeform refuses, before any device work and after everything its neighbours refuse: a missing
// motion, null or misaligned key-1 buffers, and a key-1 buffer that overlaps another buffer of the call
inline int deform_check(const TwoLevelCall& c)
{
    const char* fn = c.fn;
    const NtrInstanceDeform& d = *c.deform;
    if (!c.motion) return set_error(NTR_ERR_INVALID, "%s: null motion", fn);
    if (!d.d_poolNodes1) return set_error(NTR_ERR_INVALID, "%s: null d_poolNodes1", fn);
    if (!d.d_poolVertRows0) return set_error(NTR_ERR_INVALID, "%s: null d_poolVertRows0", fn);
    if (!d.d_poolVertRows1) return set_error(NTR_ERR_INVALID, "%s: null d_poolVertRows1", fn);
    if (((uintptr_t)d.d_poolNodes1 | (uintptr_t)d.d_poolVertRows0 | (uintptr_t)d.d_poolVertRows1) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: d_poolNodes1, d_poolVertRows0 and d_poolVertRows1 must be 16-byte aligned", fn);
    struct Span { const char* name; uintptr_t at; uint64_t bytes; };
    const uint64_t rays = (uint64_t)c.numRays, insts = (uint64_t)c.numInstances;
    const Span fresh[3] = {{"d_poolNodes1", (uintptr_t)d.d_poolNodes1, (uint64_t)c.poolNodesBytes},
                           {"d_poolVertRows0", (uintptr_t)d.d_poolVertRows0, (uint64_t)c.poolTriWoopBytes},
                           {"d_poolVertRows1", (uintptr_t)d.d_poolVertRows1, (uint64_t)c.poolTriWoopBytes}};
    const Span old[11] = {{"d_rays", (uintptr_t)c.rays, 32 * rays}, {"d_results", (uintptr_t)c.results, 16 * rays},
                          {"d_instanceIDs", (uintptr_t)c.instanceIDs, 4 * rays}, {"d_tlasNodes", (uintptr_t)c.tlas, c.tlas ? (uint64_t)c.tlasBytes : 0},
                          {"d_records", (uintptr_t)c.records, (uint64_t)kRecordBytes * insts}, {"d_poolNodes", (uintptr_t)c.poolNodes, (uint64_t)c.poolNodesBytes},
                          {"d_poolTriWoop", (uintptr_t)c.poolTriWoop, (uint64_t)c.poolTriWoopBytes},
                          {"d_poolTriIndex", (uintptr_t)c.poolTriIndex, (uint64_t)c.poolTriWoopBytes / 4},
                          {"d_motionKeys", (uintptr_t)c.motion->d_motionKeys, (uint64_t)kMotionKeyBytes * insts},
                          {"d_rayTimes", (uintptr_t)c.motion->d_rayTimes, c.motion->d_rayTimes ? 4 * rays : 0},
                          {"d_instanceMasks", c.vis ? (uintptr_t)c.vis->d_instanceMasks : 0, c.vis && c.vis->d_instanceMasks ? 4 * insts : 0}};
    auto meet = [](const Span& a, const Span& b) { return a.bytes && b.bytes && a.at < b.at + b.bytes && b.at < a.at + a.bytes; };
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 11; b++)
            if (meet(fresh[a], old[b])) return set_error(NTR_ERR_INVALID, "%s: %s overlaps %s", fn, fresh[a].name, old[b].name);
        for (int b = a + 1; b < 3; b++)
            if (meet(fresh[a], fresh[b])) return set_error(NTR_ERR_INVALID, "%s: %s overlaps %s", fn, fresh[a].name, fresh[b].name);
    }
    return NTR_OK;
}

// Zeroes the out-arguments and checks the call.  *go: the call is good and has rays to trace (NTR_OK with !*go: numRays == 0, done).
inline int two_level_check(const TwoLevelCall& c, bool* go)
{
    const char* fn = c.fn;
    *go = false;
    if (c.seconds) *c.seconds = 0.0f;
    if (c.stats) memset(c.stats, 0, sizeof(*c.stats));
    if (c.fastStats) memset(c.fastStats, 0, sizeof(*c.fastStats));
    if (c.motionStats) memset(c.motionStats, 0, sizeof(*c.motionStats));
    if (c.deformStats) memset(c.deformStats, 0, sizeof(*c.deformStats));
    if (c.validate && (c.stats != nullptr) != (c.fastStats != nullptr)) return set_error(NTR_ERR_INVALID, "%s: null stats", fn);
    if (c.numRays < 0) return set_error(NTR_ERR_INVALID, "%s: numRays < 0", fn);
    if (c.numRays == 0) return NTR_OK;
    if (!c.rays || !c.results || !c.instanceIDs) return set_error(NTR_ERR_INVALID, "%s: null ray, result or instance id buffer", fn);
    if (c.numInstances < 1 || (int64_t)c.numInstances * kRecordBytes > kPoolMaxBytes || !c.records || !c.poolNodes || !c.poolTriWoop ||
        !c.poolTriIndex)
        return set_error(NTR_ERR_INVALID, "%s: no instances or no pool", fn);
    if (const int rc = check_root_link(fn, c.rootLink, c.numInstances)) return rc;
    const TwoLevelLayout& l = c.layout;
    if (c.tlasBytes < 0 || (c.tlasBytes % l.unit) != 0 || c.tlasBytes > l.tlasMaxBytes || (c.rootLink == 0 && (!c.tlas || c.tlasBytes < l.unit)))
        return set_error(NTR_ERR_INVALID, l.tlasRefusal, fn, (unsigned long long)l.tlasMaxBytes);
    if (const int rc = check_pool_bytes(fn, l.poolNodesName, c.poolNodesBytes, l.unit)) return rc;   // (check_wide_pool_bytes's words at 128)
    if (const int rc = check_pool_bytes(fn, "poolTriWoopBytes", c.poolTriWoopBytes, kRowBytes)) return rc;
    if (c.vis && ((((uintptr_t)c.vis->d_instanceMasks) | ((uintptr_t)c.vis->d_rayMasks)) & 3u) != 0)
        return set_error(NTR_ERR_INVALID, "%s: a mask array must be 4-byte aligned", fn);
    if (c.seed == TwoLevelSeed::kRequired && (!c.seedResults || (((uintptr_t)c.seedResults) & 15u) != 0))
        return set_error(NTR_ERR_INVALID, "%s: the seed records must be given and 16-byte aligned", fn);
    if (c.seed == TwoLevelSeed::kOptional && (((uintptr_t)c.seedResults) & 15u) != 0)
        return set_error(NTR_ERR_INVALID, "%s: the seed records must be 16-byte aligned", fn);
    if (c.validate && (!c.d_flags || (((uintptr_t)c.d_flags) & 15u) != 0))
        return set_error(NTR_ERR_INVALID, "%s: the flags (%s) must be given and 16-byte aligned", fn, c.validate);
    if (c.motion && motion_check(fn, c.motion, c.numInstances) != NTR_OK) return NTR_ERR_INVALID;
    if (c.deform && deform_check(c) != NTR_OK) return NTR_ERR_INVALID;
    *go = true;
    return NTR_OK;
}

// The fields that the parameter structs of the four units name alike: the kernels' P (InstancedParams, InstancedWideParams) ...
template <class P>
void two_level_fill(P& p, const TwoLevelCall& c, DeviceState* ds)
{
    p.numRays = c.numRays; p.anyHit = c.anyHit ? 1 : 0; p.rays = c.rays; p.results = c.results; p.instanceIDs = c.instanceIDs;
    p.tlas = c.tlas; p.records = c.records; p.poolWoop = c.poolTriWoop;
    p.tlasBytes = c.tlas ? (uint32_t)c.tlasBytes : 0u; p.recordsBytes = (uint32_t)((int64_t)c.numInstances * kRecordBytes);
    p.poolWoopBytes = (uint32_t)c.poolTriWoopBytes;
    p.triIndex = c.poolTriIndex; p.rootLink = c.rootLink; p.numInstances = c.numInstances; p.status = ds->status;
}
// ... and the visibility and counter fields (InstancedExtras, InstancedWideParams).  -> a mask can refuse something: without one the
// unmasked kernel does
template <class X>
bool two_level_fill_visibility(X& x, const TwoLevelCall& c, DeviceState* ds)
{
    x.rayMask = 0xFFFFFFFFu;
    if (c.vis) {
        x.instMasks = c.vis->d_instanceMasks; x.instMasksBytes = c.vis->d_instanceMasks ? (uint32_t)((int64_t)c.numInstances * 4) : 0u;
        x.rayMasks = c.vis->d_rayMasks; x.rayMask = c.vis->rayMask;
    }
    x.stats = ds->stats;   // STATS: the seven counters, and in the FAST units [8..11] (of 32 words)
    return x.instMasks || x.rayMasks || x.rayMask != 0xFFFFFFFFu;
}

// the words an instrumented kernel adds to: [0..6], [8..11] in the FAST units, [12..13] in the motion units, [14..16] in the deform unit
constexpr int kTwoLevelCounters = 7, kTwoLevelFastCounters = 12, kTwoLevelMotionCounters = 14, kTwoLevelDeformCounters = 17;

// The shared path of the entry points.  launch(ds, stream, blocks) fills the unit's parameters and enqueues the kernel that c asks for.
template <class Launch>
int two_level_trace(const TwoLevelCall& c, Launch&& launch)
{
    bool go = false;
    if (const int rc = two_level_check(c, &go)) return rc;
    if (!go) return NTR_OK;
    DeviceState* ds = nullptr;
    if (const int rc = current_device_state_ready(&ds)) return rc;
    hipStream_t s = (hipStream_t)c.stream;
    if (c.stats && stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "%s: the call reads its counters back and cannot be captured", c.fn);
    unsigned long long h[kTwoLevelDeformCounters] = {};
    const int words = !c.stats ? 0 : c.deformStats ? kTwoLevelDeformCounters : c.motionStats ? kTwoLevelMotionCounters
                                   : c.fastStats ? kTwoLevelFastCounters : kTwoLevelCounters;
    if (const int rc = launch_trace_rays(c.fn, ds, s, c.numRays, c.seconds, words, h, [&](unsigned int blocks) { launch(ds, s, blocks); })) return rc;
    if (c.stats) {
        c.stats->numRays = c.numRays;
        c.stats->numTopInnerVisits = (int64_t)h[0]; c.stats->numInstanceEntries = (int64_t)h[1]; c.stats->numInstancesMasked = (int64_t)h[2];
        c.stats->numInnerVisits = (int64_t)h[3]; c.stats->numTriTests = (int64_t)h[4]; c.stats->numLeafVisits = (int64_t)h[5];
        c.stats->numHits = (int64_t)h[6];
    }
    if (c.fastStats) {
        c.fastStats->waveSteps = h[8]; c.fastStats->fastWaveSteps = h[9]; c.fastStats->niceStarts = h[10]; c.fastStats->niceEntries = h[11];
    }
    if (c.motionStats) { c.motionStats->numMovingEntries = (int64_t)h[12]; c.motionStats->numSingular = (int64_t)h[13]; }
    if (c.deformStats) {
        c.deformStats->numDeformEntries = (int64_t)h[14]; c.deformStats->numDeformInnerVisits = (int64_t)h[15];
        c.deformStats->numDeformTriTests = (int64_t)h[16];
    }
    return NTR_OK;
}

}  // namespace ntr
