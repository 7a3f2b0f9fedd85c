// trace_wide_kernels.hip -- the trace over a 4-wide tree for gfx950 (ntr_trace_wide, ntr_trace_wide_stats): the node buffer that
// ntr_bvh_widen writes (wide_bvh.h) over the binary tree's own Woop rows and triIndex.  EXTENSION: the reference has no wide tree; the
// rule is the numpy spec tests/np_bvh_wide.py, which the kernel equals in all four result words.  KNOWN LIMIT, as the spec states it:
// the records may differ from the binary tracer's on the same tree, because a rounded box test is not conservative and the visiting order
// decides among hits of equal t.  The spec is the definition, not the binary tracer.
// One kernel family, 64-thread workgroups, one ray per lane: a unified-step loop built from trace_lane.h and trace_wide_lane.h (the wide
// node's fetch and step, which trace_instanced_wide_kernels.hip shares).  Per iteration a lane on a wide
// node fetches rows 0..6 of its node (row 7, the child count, is for the host: a link of 0 already says that a slot is empty), a lane on a
// triangle the four rows unified_advance uses; both through wave-uniform range-checked descriptors with one wait, and a kind that no lane
// holds is skipped by a scalar branch (the shape of fetch64_two_buffers).  Whatever a link holds, a lane reads zeros and never faults.
//   wide node   ray_box2<FAST, 8> on rows (0, 1, 2) and on rows (4, 5, 6), unchanged; the three-comparison candidate test masked by
//               link != 0; a five-comparator network over (mn, k); up to three stack_push, farthest first
//   triangle    unified_advance's triangle side, unchanged
// FAST is chosen per wave as the per-ray body chooses it (NTR_BVH_FASTDIV and every live ray nice): the records are the same either way.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "wide_bvh.h"
#include "trace_launch.h"
#include "trace_lane.h"
#include "trace_wide_lane.h"

namespace ntr {
namespace {

struct WideParams {
    int32_t numRays, anyHit;
    const NtrRay* rays;
    NtrRayResult* results;
    const void *wide, *woop;
    uint32_t wideBytes, woopBytes;           // descriptor ranges (out-of-range loads return 0)
    const int32_t* triIndex;
    uint32_t bvhFlags;
    unsigned int* status;                    // sticky error bits
    unsigned long long* stats;               // STATS: {wide nodes visited, triangle tests, leaf terminators, hits}
};

template <bool FAST, bool STATS>
__device__ __forceinline__ void traverse_wide(const WideParams& p, RayRegs& r, int& node, LaneStack& st, int (&spill)[SPILL_DEPTH], int& hitAddr,
                                              float& hitU, float& hitV, LaneStats& ls)
{
    const u32x4 rWide = rsrc_words(p.wide, p.wideBytes), rWoop = rsrc_words(p.woop, p.woopBytes);
    const bool anyHit = p.anyHit != 0;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a, d = a, e = a, f = a, g = a;
    for (;;) {
        if (__ballot(node != kSentinel) == 0ull) break;
        const bool inner = (unsigned)node < (unsigned)kSentinel;
        const bool atTri = node < 0;
        const int ofs = inner ? node : leaf_row(node) * kRowBytes;
        fetch_wide_or_triangle(rWide, rWoop, ofs, __ballot(inner), __ballot(atTri), a, b, c, d, e, f, g);
        if (inner) {
            if (STATS) ls.inner++;
            wide_advance<FAST>(a, b, c, d, e, f, g, r, node, st, spill, p.status);
        } else if (atTri) {
            int row = -1;   // the row of a hit this step accepts
            unified_advance<FAST, 8>(a, b, c, d, r, node, st, spill, anyHit, row, hitU, hitV, p.status);
            if (row >= 0) hitAddr = row;
            if (STATS) {    // leaf_step's counters: a triangle test unless the row is a terminator; a terminator read unless an any-hit ray ended
                const bool term = __float_as_uint(a.x) == kLeafTerm;
                if (!term) ls.tris++;
                if (term || (!(anyHit && row >= 0) && __float_as_uint(d.x) == kLeafTerm)) ls.leaves++;
            }
        }
    }
}

template <bool STATS>
__global__ __launch_bounds__(64) void trace_wide(WideParams p)
{
    __shared__ int s_stack[LDS_DEPTH][64];   // [entry][lane]
    const int lane = threadIdx.x;
    const int rayIdx = blockIdx.x * 64 + lane;
    const bool valid = rayIdx < p.numRays;

    RayRegs r;
    load_ray(p.rays, valid ? rayIdx : 0, r);
    LaneStack st;
    int spill[SPILL_DEPTH];
    st.lds = (lds_int*)&s_stack[0][lane];
    stack_reset(st);

    int hitAddr = -1;
    float hitU = 0.0f, hitV = 0.0f;
    // a degenerate ray (Ray::degenerate, Util.hpp:65) is a miss without traversal
    int node = (valid && r.tmin < r.tmax) ? 0 : kSentinel;
    LaneStats ls = {0u, 0u, 0u};

    const bool fastWave = (p.bvhFlags & NTR_BVH_FASTDIV) && __ballot(node != kSentinel && !ray_is_nice(r, p.bvhFlags)) == 0ull;
    if (fastWave) traverse_wide<true, STATS>(p, r, node, st, spill, hitAddr, hitU, hitV, ls);
    else traverse_wide<false, STATS>(p, r, node, st, spill, hitAddr, hitU, hitV, ls);

    if (!valid) return;
    store_result(p.results, p.triIndex, rayIdx, hitAddr, r.tmax, hitU, hitV);
    if (STATS) {   // diagnostics variant only: plain per-lane atomics
        atomicAdd(&p.stats[0], (unsigned long long)ls.inner);
        atomicAdd(&p.stats[1], (unsigned long long)ls.tris);
        atomicAdd(&p.stats[2], (unsigned long long)ls.leaves);
        atomicAdd(&p.stats[3], (unsigned long long)(hitAddr >= 0));
    }
}

int trace_wide_impl(const char* fn, int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, const void* d_wideNodes,
                    int64_t wideNodesBytes, const void* d_triWoop, int64_t triWoopBytes, const int32_t* d_triIndex, uint32_t bvhFlags,
                    void* stream, float* seconds, NtrTraceStats* stats)
{
    if (seconds) *seconds = 0.0f;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (numRays < 0) return set_error(NTR_ERR_INVALID, "%s: numRays < 0", fn);
    if (numRays == 0) return NTR_OK;
    if (!d_rays || !d_results) return set_error(NTR_ERR_INVALID, "%s: null ray or result buffer", fn);
    if (!d_wideNodes || !d_triWoop || !d_triIndex) return set_error(NTR_ERR_INVALID, "%s: null BVH buffer", fn);
    if (const int rc = check_wide_bytes(fn, wideNodesBytes)) return rc;
    if (triWoopBytes < kRowBytes || (triWoopBytes % kRowBytes) != 0 || triWoopBytes > 0xFFFFFF00ll)
        return set_error(NTR_ERR_INVALID, "%s: triWoopBytes must be a multiple of 16 in [16, 0xFFFFFF00]", fn);

    DeviceState* ds = nullptr;
    if (const int rc = current_device_state_ready(&ds)) return rc;
    hipStream_t s = (hipStream_t)stream;
    WideParams p{};
    p.numRays = numRays; p.anyHit = anyHit ? 1 : 0; p.rays = d_rays; p.results = d_results;
    p.wide = d_wideNodes; p.woop = d_triWoop; p.wideBytes = (uint32_t)wideNodesBytes; p.woopBytes = (uint32_t)triWoopBytes;
    p.triIndex = d_triIndex; p.bvhFlags = bvhFlags; p.status = ds->status; p.stats = ds->stats;

    unsigned long long h[4] = {};
    const int rc = launch_trace_rays(fn, ds, s, numRays, seconds, stats ? 4 : 0, h, [&](unsigned int blocks) {
        if (stats) hipLaunchKernelGGL(trace_wide<true>, dim3(blocks), dim3(64), 0, s, p);
        else hipLaunchKernelGGL(trace_wide<false>, dim3(blocks), dim3(64), 0, s, p);
    });
    if (rc != NTR_OK) return rc;
    if (stats) {
        stats->numRays = numRays;
        stats->numInnerVisits = (int64_t)h[0]; stats->numTriTests = (int64_t)h[1]; stats->numLeafVisits = (int64_t)h[2]; stats->numHits = (int64_t)h[3];
    }
    return NTR_OK;
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" int ntr_trace_wide(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, const void* d_wideNodes,
                              int64_t wideNodesBytes, const void* d_triWoop, int64_t triWoopBytes, const int32_t* d_triIndex, uint32_t bvhFlags,
                              void* stream, float* seconds)
{
    return trace_wide_impl("ntr_trace_wide", numRays, anyHit, d_rays, d_results, d_wideNodes, wideNodesBytes, d_triWoop, triWoopBytes, d_triIndex,
                           bvhFlags, stream, seconds, nullptr);
}

extern "C" int ntr_trace_wide_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, const void* d_wideNodes,
                                    int64_t wideNodesBytes, const void* d_triWoop, int64_t triWoopBytes, const int32_t* d_triIndex,
                                    uint32_t bvhFlags, void* stream, NtrTraceStats* stats)
{
    if (!stats) return set_error(NTR_ERR_INVALID, "ntr_trace_wide_stats: null stats");
    return trace_wide_impl("ntr_trace_wide_stats", numRays, anyHit, d_rays, d_results, d_wideNodes, wideNodesBytes, d_triWoop, triWoopBytes,
                           d_triIndex, bvhFlags, stream, nullptr, stats);
}
