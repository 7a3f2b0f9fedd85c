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
// Arithmetic is the GENERIC path only, as in the binary two-level trace.  Three instantiations of the one loop:
//   trace_instanced_wide<false, false>   unmasked: vis == NULL, or a vis that can refuse nothing
//   trace_instanced_wide<true, false>    visibility masks
//   trace_instanced_wide<true, true>     the masked loop with per-lane counters (ntr_trace_instanced_wide_stats; not a timed path)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "instanced_wide_bvh.h"
#include "device_scratch.h"
#include "sched_state.h"
#include "trace_lane.h"
#include "trace_wide_lane.h"

namespace ntr {
namespace {

struct InstancedWideParams {
    int32_t numRays, anyHit;
    const NtrRay* rays;
    NtrRayResult* results;
    int32_t* instanceIDs;
    const void *tlas, *records, *poolWide, *poolWoop;
    uint32_t tlasBytes, recordsBytes, poolWideBytes, poolWoopBytes;   // descriptor ranges (out-of-range loads return 0)
    const int32_t* triIndex;
    int32_t rootLink, numInstances;
    unsigned int* status;          // sticky error bits
    const void* instMasks;         // numInstances words, or NULL: every instance 0xFFFFFFFF
    const uint32_t* rayMasks;      // numRays words, or NULL: every ray has rayMask
    uint32_t instMasksBytes, rayMask;
    unsigned long long* stats;     // STATS: {top wide nodes, entries, masked, wide nodes inside instances, triangle tests, leaf terminators, hits}
};

// Lanes of mTop fetch rows 0..6 of the wide node at byte offset `ofs` of the top-level buffer, lanes of mBot the same of the wide pool,
// into a..g; lanes of mRec the 64 bytes at `ofs` of the records and lanes of mTri those of the Woop rows into a..d; lanes of mWord (the
// entering lanes, or none) the word at `wofs` of the instance masks into w.  All range-checked (beyond the extent a load returns 0 and
// touches no memory), all under one saved exec and one wait; a group whose mask is empty is skipped by a scalar branch; the other
// lanes keep what the registers held.  The rows' loads are trace_wide_lane.h's, as in fetch_wide_or_triangle.
#define NTR_TW_GROUP(M, L, LOADS)                                           \
    "s_and_b64 exec, %[sav], %[" M "]\n\t"                                  \
    "s_cbranch_execz .Lcs_tw" L "%=\n\t"                                    \
    LOADS                                                                   \
    ".Lcs_tw" L "%=:\n\t"
__device__ __forceinline__ void fetch_two_level_wide(u32x4 rTop, u32x4 rRec, u32x4 rBot, u32x4 rTri, u32x4 rWord, int ofs, int wofs,
                                                     unsigned long long mTop, unsigned long long mRec, unsigned long long mBot,
                                                     unsigned long long mTri, unsigned long long mWord, float4& a, float4& b, float4& c,
                                                     float4& d, float4& e, float4& f, float4& g, unsigned int& w)
{
    u32x4 va = as_u4(a), vb = as_u4(b), vc = as_u4(c), vd = as_u4(d), ve = as_u4(e), vf = as_u4(f), vg = as_u4(g);
    unsigned long long sav;
    asm volatile("s_mov_b64 %[sav], exec\n\t"
                 NTR_TW_GROUP("mtop", "a", NTR_WIDE_ROWS4("rtop") NTR_WIDE_ROWS3("rtop"))
                 NTR_TW_GROUP("mrec", "b", NTR_WIDE_ROWS4("rrec"))
                 NTR_TW_GROUP("mword", "w", "buffer_load_dword %[w], %[wofs], %[rword], 0 offen\n\t")
                 NTR_TW_GROUP("mbot", "c", NTR_WIDE_ROWS4("rbot") NTR_WIDE_ROWS3("rbot"))
                 NTR_TW_GROUP("mtri", "d", NTR_WIDE_ROWS4("rtri"))
                 "s_mov_b64 exec, %[sav]\n\t"
                 "s_waitcnt vmcnt(0)"
                 : [a] "+v"(va), [b] "+v"(vb), [c] "+v"(vc), [d] "+v"(vd), [e] "+v"(ve), [f] "+v"(vf), [g] "+v"(vg), [w] "+v"(w),
                   [sav] "=&s"(sav)
                 : [ofs] "v"(ofs), [wofs] "v"(wofs), [rtop] "s"(rTop), [rrec] "s"(rRec), [rbot] "s"(rBot), [rtri] "s"(rTri), [rword] "s"(rWord),
                   [mtop] "s"(mTop), [mrec] "s"(mRec), [mbot] "s"(mBot), [mtri] "s"(mTri), [mword] "s"(mWord)
                 : "memory", "scc");   // (s_and_b64 writes SCC)
    a = as_f4(va); b = as_f4(vb); c = as_f4(vc); d = as_f4(vd); e = as_f4(ve); f = as_f4(vf); g = as_f4(vg);
}
#undef NTR_TW_GROUP

struct InstancedLaneStats {
    unsigned int topInner, entries, masked, inner, tris, leaves;
};

template <bool MASKED, bool STATS>
__global__ __launch_bounds__(64) void trace_instanced_wide(InstancedWideParams p)
{
    __shared__ int s_stack[LDS_DEPTH][64];   // [entry][lane]
    const int lane = threadIdx.x;
    const int rayIdx = blockIdx.x * 64 + lane;
    const bool valid = rayIdx < p.numRays;
    const float4* rays4 = reinterpret_cast<const float4*>(p.rays);
    const u32x4 rTlas = rsrc_words(p.tlas, p.tlasBytes), rRec = rsrc_words(p.records, p.recordsBytes),
                rWide = rsrc_words(p.poolWide, p.poolWideBytes), rWoop = rsrc_words(p.poolWoop, p.poolWoopBytes);
    const bool anyHit = p.anyHit != 0;
    u32x4 rMasks = rTlas;
    unsigned int rayMask = 0xFFFFFFFFu;   // m_r
    bool instMasks = false;               // wave-uniform: without instance masks no entering step loads a word
    if (MASKED) {
        rMasks = rsrc_words(p.instMasks, p.instMasksBytes);
        instMasks = p.instMasks != nullptr;
        rayMask = p.rayMasks ? p.rayMasks[valid ? rayIdx : 0] : p.rayMask;
    }
    InstancedLaneStats ls = {0u, 0u, 0u, 0u, 0u, 0u};

    RayRegs r;   // the current form: the world ray on the top level, the object ray inside an instance
    {
        const float4 o = rays4[(valid ? rayIdx : 0) * 2 + 0], d = rays4[(valid ? rayIdx : 0) * 2 + 1];
        r.ox = o.x; r.oy = o.y; r.oz = o.z; r.tmin = o.w;
        r.dx = d.x; r.dy = d.y; r.dz = d.z; r.tmax = d.w;
        r.rx = r.ry = r.rz = 0.0f;   // (the FAST path's reciprocals: unused)
    }
    LaneStack st;
    int spill[SPILL_DEPTH];
    st.lds = (lds_int*)&s_stack[0][lane];
    stack_reset(st);

    int hitAddr = -1, hitInst = -1;   // the hit's row in the pool's triWoop and its instance
    float hitU = 0.0f, hitV = 0.0f;
    int inst = -1;                    // >= 0: inside that instance
    unsigned int wideOffset = 0u, rowOffset = 0u, extent = 0u;
    // a degenerate ray (Ray::degenerate, Util.hpp:65) is a miss without traversal
    int node = (valid && r.tmin < r.tmax) ? p.rootLink : kSentinel;

    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a, d = a, e = a, f = a, g = a;
    for (;;) {
        if (__ballot(node != kSentinel) == 0ull) break;
        const bool top = inst < 0;
        const bool inner = (unsigned)node < (unsigned)kSentinel;
        const bool neg = node < 0;
        int ofs = kNoNode;
        if (top) {
            if (inner) ofs = node;
            else if (neg && (unsigned)~node < (unsigned)p.numInstances) ofs = ~node * kRecordBytes;
        } else if (inner) {
            // below the BLAS's extent only (node and extent are multiples of 128 in a well-formed tree: the whole node lies inside)
            const unsigned int o = wideOffset + (unsigned)node;
            if ((unsigned)node < extent && o >= wideOffset && o < (unsigned)kNoNode) ofs = (int)o;   // (a sum that wraps reads nothing)
        } else if (neg) {
            const unsigned int row = rowOffset + (unsigned)~node;
            if (row < (unsigned)(kPoolMaxBytes >> kRowShift)) ofs = (int)(row << kRowShift);
        }
        unsigned int instMask = 0xFFFFFFFFu;   // M_i of an entering lane
        {
            // the word of record ofs / 64 lies at ofs / 16; an entering lane whose index is out of range holds kNoNode, and kNoNode / 16 =
            // 0x0FFFFFF0 is at or beyond the end of any mask array (4 * numInstances <= kPoolMaxBytes / 16): it reads 0 and touches nothing
            const unsigned long long enter = __ballot(top && neg);
            fetch_two_level_wide(rTlas, rRec, rWide, rWoop, rMasks, ofs, (int)((unsigned)ofs >> 4), __ballot(top && inner), enter,
                                 __ballot(!top && inner), __ballot(!top && neg), (MASKED && instMasks) ? enter : 0ull, a, b, c, d, e, f, g,
                                 instMask);
        }
        if (node == kSentinel) {
            // done: waits for the wave
        } else if (!inner && !neg) {
            // a positive word above the sentinel: the exit marker.  Leaving: the world ray again (tmin and the shrunk tmax stay)
            if (node == kExitMarker) {
                const float4 o = rays4[rayIdx * 2 + 0], dd = rays4[rayIdx * 2 + 1];
                r.ox = o.x; r.oy = o.y; r.oz = o.z;
                r.dx = dd.x; r.dy = dd.y; r.dz = dd.z;
                inst = -1;
            }
            node = stack_pop(st, spill);   // (any other such word is no link: it is dropped)
        } else if (inner) {
            // a wide node of either level (a lane whose fetch lay beyond an extent read zeros: four links of 0, no candidate, a pop)
            if (STATS) { if (top) ls.topInner++; else ls.inner++; }
            wide_advance<false>(a, b, c, d, e, f, g, r, node, st, spill, p.status);
        } else if (top) {
            // entering instance ~node: its record is worldToObject (a, b, c) and the wide offset, row offset and extent (d)
            const int idx = ~node;
            if ((unsigned)idx >= (unsigned)p.numInstances) {
                node = stack_pop(st, spill);
            } else if (MASKED && (instMask & rayMask) == 0u) {
                if (STATS) ls.masked++;
                node = stack_pop(st, spill);         // refused: no marker, no transform; the fetched record is dropped
            } else if (st.sp >= LDS_DEPTH + SPILL_DEPTH) {
                atomicOr(p.status, NTR_STATUS_STACK_OVERFLOW);   // no room for the marker: the instance is not entered
                node = stack_pop(st, spill);
            } else {
                stack_push(st, spill, kExitMarker, p.status);
                const float ox = dot4(a, r.ox, r.oy, r.oz, 1.0f), oy = dot4(b, r.ox, r.oy, r.oz, 1.0f), oz = dot4(c, r.ox, r.oy, r.oz, 1.0f);
                const float dx = dot4(a, r.dx, r.dy, r.dz, 0.0f), dy = dot4(b, r.dx, r.dy, r.dz, 0.0f), dz = dot4(c, r.dx, r.dy, r.dz, 0.0f);
                r.ox = ox; r.oy = oy; r.oz = oz;
                r.dx = dx; r.dy = dy; r.dz = dz;
                wideOffset = __float_as_uint(d.x);
                rowOffset = __float_as_uint(d.y);
                extent = __float_as_uint(d.z);
                inst = idx;
                node = 0;
                if (STATS) ls.entries++;
            }
        } else {
            int row = -1;   // the BLAS's own row of a hit this step accepts
            if (STATS) {
                // leaf_step's counters: a triangle test unless the row is a terminator; a terminator read for the row itself or for the word
                // that came with a triangle -- unless an any-hit ray ended on that triangle
                const bool term = __float_as_uint(a.x) == kLeafTerm;
                if (!term) ls.tris++;
                unified_advance<false, 8>(a, b, c, d, r, node, st, spill, anyHit, row, hitU, hitV, p.status);
                if (term || (!(anyHit && row >= 0) && __float_as_uint(d.x) == kLeafTerm)) ls.leaves++;
            } else {
                unified_advance<false, 8>(a, b, c, d, r, node, st, spill, anyHit, row, hitU, hitV, p.status);
            }
            if (row >= 0) {
                hitAddr = (int)(rowOffset + (unsigned)row);
                hitInst = inst;
            }
        }
    }
    if (!valid) return;
    store_result(p.results, p.triIndex, rayIdx, hitAddr, r.tmax, hitU, hitV);
    p.instanceIDs[rayIdx] = hitInst;
    if (STATS) {   // diagnostics variant only: plain per-lane atomics
        atomicAdd(&p.stats[0], (unsigned long long)ls.topInner);
        atomicAdd(&p.stats[1], (unsigned long long)ls.entries);
        atomicAdd(&p.stats[2], (unsigned long long)ls.masked);
        atomicAdd(&p.stats[3], (unsigned long long)ls.inner);
        atomicAdd(&p.stats[4], (unsigned long long)ls.tris);
        atomicAdd(&p.stats[5], (unsigned long long)ls.leaves);
        atomicAdd(&p.stats[6], (unsigned long long)(hitAddr >= 0 && p.triIndex[hitAddr] != -1));
    }
}

// The two entry points' one body.  vis == NULL, or a vis that can refuse nothing (no arrays and rayMask all ones), launches the unmasked
// kernel; stats != NULL launches the instrumented one and reads the counters back.
int trace_instanced_wide_impl(const char* fn, int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                              int32_t* d_instanceIDs, const void* d_wideTlasNodes, int64_t wideTlasNodesBytes, int32_t rootLink,
                              const void* d_wideRecords, int32_t numInstances, const void* d_widePoolNodes, int64_t widePoolNodesBytes,
                              const void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                              const NtrInstanceVisibility* vis, float* seconds, void* stream, NtrInstancedTraceStats* stats)
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
    if (stats) {
        NTR_HIP(hipMemsetAsync(ds->stats, 0, 7 * sizeof(unsigned long long), s));
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
