// trace_motion_kernels.hip -- the time-sampled trace over ONE Compact tree whose boxes and triangles move between two keys, for gfx950
// (ntr_trace_bvh_motion, ntr_trace_bvh_motion_stats): deformation motion blur.  EXTENSION: the reference's scenes are static; the rule is
// the numpy spec tests/np_bvh_motion.py, which the kernel equals in all four result words and every counter.  The buffers are
// ntr_bvh_motion_refit's: the two keys' node buffers (links from key 0) and the two keys' vertex rows.
// One kernel family in the shape of trace_wide_kernels.hip: 64-thread workgroups, one ray per lane, trace_lane.h's ray, stack and result,
// a unified-step loop.  Per iteration a lane on an inner node fetches rows 0..3 of its node from nodes0 and rows 0..2 from nodes1; a lane
// on a triangle its three vertex rows from either key and the w word of the row behind them; all through wave-uniform range-checked
// descriptors with one wait, and a kind that no lane holds is skipped by a scalar branch.  Whatever a link holds, a lane reads zeros and
// never faults.
//   inner node  the twelve box words posed by motion_deform_lerp, then inner_advance<false, 8> (ray_box2<false, 8>), unchanged.  There
//               is no FAST form: ntr_bvh_validate's flags say nothing about lerped boxes
//   triangle    a terminator iff the W word of the first row is 0x80000000 (a vertex's x may be -0.0f, the same word); otherwise the
//               nine vertex words posed by motion_deform_lerp, woop_rows_verts (its binary64 reciprocal is what makes the two ends equal
//               the refit's rows) and triangle_step, unchanged
// The pose is NOT instance_motion.h's motion_lerp: it has no "same word" shortcut, so that the posed box contains the posed triangle
// exactly (the spec's docstring says why).  Compiled with the library's flags: no contraction.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "compact_bvh.h"
#include "instance_motion.h"
#include "trace_launch.h"
#include "trace_lane.h"
#include "trace_deform_pose.h"
#include "woop_rows.h"

namespace ntr {
namespace {

struct MotionParams {
    int32_t numRays, anyHit;
    const NtrRay* rays;
    NtrRayResult* results;
    const void *nodes0, *nodes1, *verts0, *verts1;
    uint32_t nodesBytes, vertsBytes;         // descriptor ranges, each for both keys (out-of-range loads return 0)
    const int32_t* triIndex;
    const float* rayTimes;                   // or null: every ray has `time`
    float time;
    unsigned int* status;                    // sticky error bits
    unsigned long long* stats;               // STATS: {inner nodes visited, triangle tests, leaf terminators, hits}
};

// motion_deform_lerp, deform_lerp of the spec per word, is trace_deform_pose.h's, shared with the two-level unit

// Lanes of maskN fetch rows 0..3 of the node at byte offset `ofs` of nodes0 into a..d and rows 0..2 of nodes1 into e..g; lanes of maskT
// rows 0..2 at `ofs` of verts0 into a..c, of verts1 into e..g, and the w word of verts0's row behind them into nextW (range-checked:
// beyond the extent a load returns 0 and touches no memory); the other lanes keep what the registers held.
#define NTR_MOTION_ROWS3(A, B, C, R)                                        \
    "buffer_load_dwordx4 %[" A "], %[ofs], %[" R "], 0 offen\n\t"           \
    "buffer_load_dwordx4 %[" B "], %[ofs], %[" R "], 0 offen offset:16\n\t" \
    "buffer_load_dwordx4 %[" C "], %[ofs], %[" R "], 0 offen offset:32\n\t"
__device__ __forceinline__ void fetch_motion_node_or_triangle(u32x4 rNodes0, u32x4 rNodes1, u32x4 rVerts0, u32x4 rVerts1, int ofs,
                                                              unsigned long long maskN, unsigned long long maskT, float4& a, float4& b,
                                                              float4& c, float4& d, float4& e, float4& f, float4& g, unsigned int& nextW)
{
    u32x4 va = as_u4(a), vb = as_u4(b), vc = as_u4(c), vd = as_u4(d), ve = as_u4(e), vf = as_u4(f), vg = as_u4(g);
    unsigned long long sav;
    asm volatile("s_mov_b64 %[sav], exec\n\t"
                 "s_and_b64 exec, %[sav], %[mn]\n\t"
                 "s_cbranch_execz .Lmo_fetch_n%=\n\t"
                 NTR_MOTION_ROWS3("a", "b", "c", "n0")
                 "buffer_load_dwordx4 %[d], %[ofs], %[n0], 0 offen offset:48\n\t"
                 NTR_MOTION_ROWS3("e", "f", "g", "n1")
                 ".Lmo_fetch_n%=:\n\t"
                 "s_and_b64 exec, %[sav], %[mt]\n\t"
                 "s_cbranch_execz .Lmo_fetch_t%=\n\t"
                 NTR_MOTION_ROWS3("a", "b", "c", "v0")
                 "buffer_load_dword %[nw], %[ofs], %[v0], 0 offen offset:60\n\t"
                 NTR_MOTION_ROWS3("e", "f", "g", "v1")
                 ".Lmo_fetch_t%=:\n\t"
                 "s_mov_b64 exec, %[sav]\n\t"
                 "s_waitcnt vmcnt(0)"
                 : [a] "+v"(va), [b] "+v"(vb), [c] "+v"(vc), [d] "+v"(vd), [e] "+v"(ve), [f] "+v"(vf), [g] "+v"(vg), [nw] "+v"(nextW),
                   [sav] "=&s"(sav)
                 : [ofs] "v"(ofs), [n0] "s"(rNodes0), [n1] "s"(rNodes1), [v0] "s"(rVerts0), [v1] "s"(rVerts1), [mn] "s"(maskN), [mt] "s"(maskT)
                 : "memory", "scc");   // (s_and_b64 writes SCC)
    a = as_f4(va); b = as_f4(vb); c = as_f4(vc); d = as_f4(vd); e = as_f4(ve); f = as_f4(vf); g = as_f4(vg);
}
#undef NTR_MOTION_ROWS3

template <bool STATS>
__global__ __launch_bounds__(64) void trace_bvh_motion(MotionParams p)
{
    __shared__ int s_stack[LDS_DEPTH][64];   // [entry][lane]
    const int lane = threadIdx.x;
    const int rayIdx = blockIdx.x * 64 + lane;
    const bool valid = rayIdx < p.numRays;

    RayRegs r;
    load_ray(p.rays, valid ? rayIdx : 0, r);
    const float t = motion_clamp_time(p.rayTimes ? p.rayTimes[valid ? rayIdx : 0] : p.time);
    const float u = 1.0f - t;
    LaneStack st;
    int spill[SPILL_DEPTH];
    st.lds = (lds_int*)&s_stack[0][lane];
    stack_reset(st);

    int hitAddr = -1;
    float hitU = 0.0f, hitV = 0.0f;
    // a degenerate ray (Ray::degenerate, Util.hpp:65) is a miss without traversal
    int node = (valid && r.tmin < r.tmax) ? 0 : kSentinel;
    LaneStats ls = {0u, 0u, 0u};

    const u32x4 rNodes0 = rsrc_words(p.nodes0, p.nodesBytes), rNodes1 = rsrc_words(p.nodes1, p.nodesBytes);
    const u32x4 rVerts0 = rsrc_words(p.verts0, p.vertsBytes), rVerts1 = rsrc_words(p.verts1, p.vertsBytes);
    const bool anyHit = p.anyHit != 0;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a, d = a, e = a, f = a, g = a;
    unsigned int nextW = 0u;
    for (;;) {
        if (__ballot(node != kSentinel) == 0ull) break;
        const bool inner = (unsigned)node < (unsigned)kSentinel;
        const bool atTri = node < 0;
        const int ofs = inner ? node : leaf_row(node) * kRowBytes;
        fetch_motion_node_or_triangle(rNodes0, rNodes1, rVerts0, rVerts1, ofs, __ballot(inner), __ballot(atTri), a, b, c, d, e, f, g, nextW);
        if (inner) {
            if (STATS) ls.inner++;
            const float4 n0 = motion_deform_lerp4(a, e, t, u), n1 = motion_deform_lerp4(b, f, t, u), nz = motion_deform_lerp4(c, g, t, u);
            inner_advance<false, 8>(n0, n1, nz, d, r, node, st, spill, p.status);
        } else if (atTri) {
            bool leafDone = __float_as_uint(a.w) == kLeafTerm;   // terminator: an empty leaf
            if (!leafDone) {
                if (STATS) ls.tris++;
                float4 w0, w1, w2;
                woop_rows_verts(motion_deform_lerp(a.x, e.x, t, u), motion_deform_lerp(a.y, e.y, t, u), motion_deform_lerp(a.z, e.z, t, u),
                                motion_deform_lerp(b.x, f.x, t, u), motion_deform_lerp(b.y, f.y, t, u), motion_deform_lerp(b.z, f.z, t, u),
                                motion_deform_lerp(c.x, g.x, t, u), motion_deform_lerp(c.y, g.y, t, u), motion_deform_lerp(c.z, g.z, t, u),
                                w0, w1, w2);
                bool terminated = false;
                if (triangle_step(w0, w1, w2, r, hitU, hitV)) {
                    hitAddr = leaf_row(node);
                    terminated = anyHit;
                }
                if (terminated) node = kSentinel;
                else if (nextW == kLeafTerm) leafDone = true;   // the terminator came with this triangle
                else node -= kTriRows;
            }
            if (leafDone) {
                if (STATS) ls.leaves++;
                node = stack_pop(st, spill);
            }
        } else {
            node = kSentinel;   // a link beyond the sentinel (a malformed tree) names nothing: the ray ends, the loop does too
        }
    }

    if (!valid) return;
    store_result(p.results, p.triIndex, rayIdx, hitAddr, r.tmax, hitU, hitV);
    if (STATS) {   // diagnostics variant only: plain per-lane atomics
        atomicAdd(&p.stats[0], (unsigned long long)ls.inner);
        atomicAdd(&p.stats[1], (unsigned long long)ls.tris);
        atomicAdd(&p.stats[2], (unsigned long long)ls.leaves);
        atomicAdd(&p.stats[3], (unsigned long long)(hitAddr >= 0));
    }
}

int trace_motion_impl(const char* fn, int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, const void* d_nodes0,
                      int64_t nodesBytes, int64_t vertRowsBytes, const int32_t* d_triIndex, const NtrBvhMotion* motion, void* stream,
                      float* seconds, NtrTraceStats* stats)
{
    if (seconds) *seconds = 0.0f;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (numRays < 0) return set_error(NTR_ERR_INVALID, "%s: numRays < 0", fn);
    if (numRays == 0) return NTR_OK;
    if (!d_rays || !d_results) return set_error(NTR_ERR_INVALID, "%s: null ray or result buffer", fn);
    if (!motion) return set_error(NTR_ERR_INVALID, "%s: null motion", fn);
    if (!d_nodes0 || !d_triIndex || !motion->d_nodes1 || !motion->d_vertRows0 || !motion->d_vertRows1)
        return set_error(NTR_ERR_INVALID, "%s: null BVH buffer (d_nodes0, d_triIndex, motion's d_nodes1, d_vertRows0, d_vertRows1)", fn);
    if (const int rc = check_nodes_bytes(fn, "nodesBytes", nodesBytes)) return rc;
    if (vertRowsBytes < kRowBytes || (vertRowsBytes % kRowBytes) != 0 || vertRowsBytes > 0xFFFFFF00ll)
        return set_error(NTR_ERR_INVALID, "%s: vertRowsBytes must be a multiple of 16 in [16, 0xFFFFFF00]", fn);
    if ((((uintptr_t)motion->d_rayTimes) & 3u) != 0) return set_error(NTR_ERR_INVALID, "%s: the ray times must be 4-byte aligned", fn);

    DeviceState* ds = nullptr;
    if (const int rc = current_device_state_ready(&ds)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (stats && stream_is_capturing(s)) return set_error(NTR_ERR_INVALID, "%s: the call reads its counters back and cannot be captured", fn);
    MotionParams p{};
    p.numRays = numRays; p.anyHit = anyHit ? 1 : 0; p.rays = d_rays; p.results = d_results;
    p.nodes0 = d_nodes0; p.nodes1 = motion->d_nodes1; p.verts0 = motion->d_vertRows0; p.verts1 = motion->d_vertRows1;
    p.nodesBytes = (uint32_t)nodesBytes; p.vertsBytes = (uint32_t)vertRowsBytes;
    p.triIndex = d_triIndex; p.rayTimes = motion->d_rayTimes; p.time = motion->time; p.status = ds->status; p.stats = ds->stats;

    unsigned long long h[4] = {};
    const int rc = launch_trace_rays(fn, ds, s, numRays, seconds, stats ? 4 : 0, h, [&](unsigned int blocks) {
        if (stats) hipLaunchKernelGGL(trace_bvh_motion<true>, dim3(blocks), dim3(64), 0, s, p);
        else hipLaunchKernelGGL(trace_bvh_motion<false>, dim3(blocks), dim3(64), 0, s, p);
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

extern "C" int ntr_trace_bvh_motion(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, const void* d_nodes0,
                                    int64_t nodesBytes, int64_t vertRowsBytes, const int32_t* d_triIndex, const NtrBvhMotion* motion,
                                    void* stream, float* seconds)
{
    return trace_motion_impl("ntr_trace_bvh_motion", numRays, anyHit, d_rays, d_results, d_nodes0, nodesBytes, vertRowsBytes, d_triIndex, motion,
                             stream, seconds, nullptr);
}

extern "C" int ntr_trace_bvh_motion_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, const void* d_nodes0,
                                          int64_t nodesBytes, int64_t vertRowsBytes, const int32_t* d_triIndex, const NtrBvhMotion* motion,
                                          void* stream, NtrTraceStats* stats)
{
    if (!stats) return set_error(NTR_ERR_INVALID, "ntr_trace_bvh_motion_stats: null stats");
    return trace_motion_impl("ntr_trace_bvh_motion_stats", numRays, anyHit, d_rays, d_results, d_nodes0, nodesBytes, vertRowsBytes, d_triIndex,
                             motion, stream, nullptr, stats);
}
