// trace_wide_kernels.hip -- the trace over a 4-wide tree for gfx950 (ntr_trace_wide, ntr_trace_wide_stats): the node buffer that
// ntr_bvh_widen writes (wide_bvh.h) over the binary tree's own Woop rows and triIndex.  EXTENSION: the reference has no wide tree; the
// rule is the numpy spec tests/np_bvh_wide.py, which the kernel equals in all four result words.  KNOWN LIMIT, as the spec states it:
// the records may differ from the binary tracer's on the same tree, because a rounded box test is not conservative and the visiting order
// decides among hits of equal t.  The spec is the definition, not the binary tracer.
// One kernel family, 64-thread workgroups, one ray per lane: a unified-step loop built from trace_lane.h.  Per iteration a lane on a wide
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
#include "device_scratch.h"
#include "sched_state.h"
#include "trace_lane.h"

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

// Lanes of maskN fetch rows 0..6 of the wide node at byte offset `ofs` into a..g, lanes of maskT the 64 bytes at `ofs` of the Woop rows
// into a..d (range-checked: beyond the extent a load returns 0 and touches no memory); the other lanes keep what the registers held.
__device__ __forceinline__ void fetch_wide_or_triangle(u32x4 rWide, u32x4 rWoop, int ofs, unsigned long long maskN, unsigned long long maskT,
                                                       float4& a, float4& b, float4& c, float4& d, float4& e, float4& f, float4& g)
{
    u32x4 va = as_u4(a), vb = as_u4(b), vc = as_u4(c), vd = as_u4(d), ve = as_u4(e), vf = as_u4(f), vg = as_u4(g);
    unsigned long long sav;
    asm volatile("s_mov_b64 %[sav], exec\n\t"
                 "s_and_b64 exec, %[sav], %[mn]\n\t"
                 "s_cbranch_execz .Lwd_fetch_n%=\n\t"
                 "buffer_load_dwordx4 %[a], %[ofs], %[rn], 0 offen\n\t"
                 "buffer_load_dwordx4 %[b], %[ofs], %[rn], 0 offen offset:16\n\t"
                 "buffer_load_dwordx4 %[c], %[ofs], %[rn], 0 offen offset:32\n\t"
                 "buffer_load_dwordx4 %[d], %[ofs], %[rn], 0 offen offset:48\n\t"
                 "buffer_load_dwordx4 %[e], %[ofs], %[rn], 0 offen offset:64\n\t"
                 "buffer_load_dwordx4 %[f], %[ofs], %[rn], 0 offen offset:80\n\t"
                 "buffer_load_dwordx4 %[g], %[ofs], %[rn], 0 offen offset:96\n\t"
                 ".Lwd_fetch_n%=:\n\t"
                 "s_and_b64 exec, %[sav], %[mt]\n\t"
                 "s_cbranch_execz .Lwd_fetch_t%=\n\t"
                 "buffer_load_dwordx4 %[a], %[ofs], %[rt], 0 offen\n\t"
                 "buffer_load_dwordx4 %[b], %[ofs], %[rt], 0 offen offset:16\n\t"
                 "buffer_load_dwordx4 %[c], %[ofs], %[rt], 0 offen offset:32\n\t"
                 "buffer_load_dwordx4 %[d], %[ofs], %[rt], 0 offen offset:48\n\t"
                 ".Lwd_fetch_t%=:\n\t"
                 "s_mov_b64 exec, %[sav]\n\t"
                 "s_waitcnt vmcnt(0)"
                 : [a] "+v"(va), [b] "+v"(vb), [c] "+v"(vc), [d] "+v"(vd), [e] "+v"(ve), [f] "+v"(vf), [g] "+v"(vg), [sav] "=&s"(sav)
                 : [ofs] "v"(ofs), [rn] "s"(rWide), [rt] "s"(rWoop), [mn] "s"(maskN), [mt] "s"(maskT)
                 : "memory", "scc");   // (s_and_b64 writes SCC)
    a = as_f4(va); b = as_f4(vb); c = as_f4(vc); d = as_f4(vd); e = as_f4(ve); f = as_f4(vf); g = as_f4(vg);
}

// compare-exchange on (mn, k, link): afterwards the pair is in ascending (mn, k).  No mn is a NaN here, and k differs, so the order is total.
__device__ __forceinline__ void order2(float& mA, int& kA, int& lA, float& mB, int& kB, int& lB)
{
    const bool swp = mA > mB || (mA == mB && kA > kB);
    const float m = swp ? mB : mA; mB = swp ? mA : mB; mA = m;
    const int k = swp ? kB : kA; kB = swp ? kA : kB; kA = k;
    const int l = swp ? lB : lA; lB = swp ? lA : lB; lA = l;
}

// One wide node of the spec: the four boxes, the candidates in ascending (mn, k), the nearest first and the others pushed farthest first
template <bool FAST>
__device__ __forceinline__ void wide_advance(const float4& a, const float4& b, const float4& c, const float4& d, const float4& e, const float4& f,
                                             const float4& g, const RayRegs& r, int& node, LaneStack& st, int (&spill)[SPILL_DEPTH],
                                             unsigned int* status)
{
    float mn[4], mx[4];
    ray_box2<FAST, 8>(r, a, b, c, mn[0], mx[0], mn[1], mx[1]);
    ray_box2<FAST, 8>(r, e, f, g, mn[2], mx[2], mn[3], mx[3]);
    int link[4] = {__float_as_int(d.x), __float_as_int(d.y), __float_as_int(d.z), __float_as_int(d.w)};
    int k[4];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const bool cand = link[i] != 0 && (mn[i] <= mx[i]) && (mx[i] >= r.tmin) && (mn[i] <= r.tmax);
        n += cand ? 1 : 0;
        // a slot that is no candidate sorts behind every candidate: +inf, and a k above the candidates' (a candidate's mn may be +inf too)
        mn[i] = cand ? mn[i] : __builtin_inff();
        k[i] = cand ? i : i + 4;
    }
    order2(mn[0], k[0], link[0], mn[1], k[1], link[1]);
    order2(mn[2], k[2], link[2], mn[3], k[3], link[3]);
    order2(mn[0], k[0], link[0], mn[2], k[2], link[2]);
    order2(mn[1], k[1], link[1], mn[3], k[3], link[3]);
    order2(mn[1], k[1], link[1], mn[2], k[2], link[2]);
    if (n > 3) stack_push(st, spill, link[3], status);
    if (n > 2) stack_push(st, spill, link[2], status);
    if (n > 1) stack_push(st, spill, link[1], status);
    node = n > 0 ? link[0] : stack_pop(st, spill);
}

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

    StreamEvents<2> ev(s);   // the timed bracket
    if (seconds) {
        NTR_HIP(ev.create());
        NTR_HIP(hipStreamSynchronize(s));
        NTR_HIP(ev.record(0));
    }
    const dim3 grid((numRays + 63) / 64), block(64);
    if (stats) {
        NTR_HIP(hipMemsetAsync(ds->stats, 0, 4 * sizeof(unsigned long long), s));
        hipLaunchKernelGGL(trace_wide<true>, grid, block, 0, s, p);
    } else {
        hipLaunchKernelGGL(trace_wide<false>, grid, block, 0, s, p);
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
        unsigned long long h[4];
        NTR_HIP(hipMemcpyAsync(h, ds->stats, sizeof(h), hipMemcpyDeviceToHost, s));
        NTR_HIP(hipStreamSynchronize(s));
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
