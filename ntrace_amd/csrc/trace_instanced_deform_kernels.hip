// trace_instanced_deform_kernels.hip -- the motion-blurred two-level trace over a pool in which some BLASes deform, for gfx950
// (ntr_trace_instanced_deform, ntr_trace_instanced_deform_stats; the rule is tests/np_instanced_deform.py):
// trace_instanced_body.h with NTR_TI_DEFORM on top of NTR_TI_MASKED and NTR_TI_MOTION -- the motion kernel's loop, and the bottom-level
// steps of trace_motion_kernels.hip at a pool offset for the lanes that are inside a deforming BLAS.
//   deform  bit 1 of word 15 of the entered record, which ntr_tlas_deform_refit (tlas_deform_refit_kernels.hip) sets; one bit per lane,
//           set on entering and cleared at the exit marker.  Bit 0 alone decides the instance's pose, as in the motion kernel
//   fetch   the loop's four-buffer fetch stays; a deforming triangle lane is taken out of its Woop mask (a deforming BLAS's Woop rows are
//           key 0's and are not read).  Behind ONE wave-uniform branch on the ballot of the lanes inside a deforming BLAS a second
//           fetch (fetch_deform_rows, one wait) brings rows 0..2 of the node in the second key's buffer for an inner lane, and for a
//           triangle lane three rows of each key's vertex rows and the w word of the row behind them.  All through range-checked
//           descriptors with the pool's node and row extents: whatever a link holds, a lane reads zeros and never faults
//   pose    motion_deform_lerp (trace_deform_pose.h) per word; an inner lane poses its box words in place and takes the unchanged
//           step with the wave's other lanes; a triangle lane forms the Woop rows (woop_rows.h) and calls the unchanged triangle_step.
//           The terminator of a deforming leaf is the W word of key 0's vertex row
//   cost    a wave with no lane inside a deforming BLAS executes the motion kernel's iteration after the one scalar branch
// Two kernels, trace_instanced_deform and its instrumented variant (counters [14..16]: deforming entries, inner visits, triangle tests),
// in a unit of their own (trace_instanced_kernels.h: why).  The launch around them is trace_instanced_launch.h's, whose seventh client
// this is.  With deform == NULL the entry points hand the call to ntr_trace_instanced_motion / ntr_trace_instanced_motion_stats.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "ntr_internal.h"
#include "instance_math.h"
#include "instance_motion.h"
#include "instanced_bvh.h"
#include "trace_instanced_launch.h"
#include "trace_lane.h"
#include "trace_fetch.h"
#include "trace_instanced_kernels.h"
#include "trace_motion_pose.h"
#include "trace_deform_pose.h"
#include "woop_rows.h"

namespace ntr {
namespace {

// What the deform kernels take beside the motion kernels' parameters: the pool's key-1 buffers.  Their extents are the pool's
// (InstancedParams::poolNodesBytes for nodes1, poolWoopBytes for the vertex rows)
struct InstancedDeform {
    const void *nodes1, *verts0, *verts1;
};

// Lanes of maskN fetch rows 0..2 at byte offset `ofs` of nodes1 into e..g (their a..d hold the first key's node); lanes of maskT rows
// 0..2 at `ofs` of verts0 into a..c, of verts1 into e..g, and the w word of verts0's row behind them into nextW (range-checked: beyond
// the extent a load returns 0 and touches no memory); the other lanes keep what the registers held.  One wait.
#define NTR_DEFORM_ROWS3(A, B, C, R)                                        \
    "buffer_load_dwordx4 %[" A "], %[ofs], %[" R "], 0 offen\n\t"           \
    "buffer_load_dwordx4 %[" B "], %[ofs], %[" R "], 0 offen offset:16\n\t" \
    "buffer_load_dwordx4 %[" C "], %[ofs], %[" R "], 0 offen offset:32\n\t"
__device__ __forceinline__ void fetch_deform_rows(u32x4 rNodes1, u32x4 rVerts0, u32x4 rVerts1, int ofs, unsigned long long maskN,
                                                  unsigned long long maskT, float4& a, float4& b, float4& c, float4& e, float4& f, float4& g,
                                                  unsigned int& nextW)
{
    u32x4 va = as_u4(a), vb = as_u4(b), vc = as_u4(c), ve = as_u4(e), vf = as_u4(f), vg = as_u4(g);
    unsigned long long sav;
    asm volatile("s_mov_b64 %[sav], exec\n\t"
                 "s_and_b64 exec, %[sav], %[mn]\n\t"
                 "s_cbranch_execz .Lcs_dfn%=\n\t"
                 NTR_DEFORM_ROWS3("e", "f", "g", "n1")
                 ".Lcs_dfn%=:\n\t"
                 "s_and_b64 exec, %[sav], %[mt]\n\t"
                 "s_cbranch_execz .Lcs_dft%=\n\t"
                 NTR_DEFORM_ROWS3("a", "b", "c", "v0")
                 "buffer_load_dword %[nw], %[ofs], %[v0], 0 offen offset:60\n\t"
                 NTR_DEFORM_ROWS3("e", "f", "g", "v1")
                 ".Lcs_dft%=:\n\t"
                 "s_mov_b64 exec, %[sav]\n\t"
                 "s_waitcnt vmcnt(0)"
                 : [a] "+v"(va), [b] "+v"(vb), [c] "+v"(vc), [e] "+v"(ve), [f] "+v"(vf), [g] "+v"(vg), [nw] "+v"(nextW), [sav] "=&s"(sav)
                 : [ofs] "v"(ofs), [n1] "s"(rNodes1), [v0] "s"(rVerts0), [v1] "s"(rVerts1), [mn] "s"(maskN), [mt] "s"(maskT)
                 : "memory", "scc");   // (s_and_b64 writes SCC)
    a = as_f4(va); b = as_f4(vb); c = as_f4(vc); e = as_f4(ve); f = as_f4(vf); g = as_f4(vg);
}
#undef NTR_DEFORM_ROWS3

#define NTR_TI_PARAMS InstancedParams p, InstancedExtras x, InstancedMotion mo, InstancedDeform df
#define NTR_TI_MASKED 1
#define NTR_TI_SEEDED 0
#define NTR_TI_FAST 0
#define NTR_TI_MOTION 1
#define NTR_TI_DEFORM 1

#define NTR_TI_KERNEL trace_instanced_deform
#define NTR_TI_STATS 0
#include "trace_instanced_body.h"
#undef NTR_TI_KERNEL
#undef NTR_TI_STATS

#define NTR_TI_KERNEL trace_instanced_deform_stats
#define NTR_TI_STATS 1
#include "trace_instanced_body.h"
#undef NTR_TI_KERNEL
#undef NTR_TI_STATS

#undef NTR_TI_PARAMS
#undef NTR_TI_MASKED
#undef NTR_TI_SEEDED
#undef NTR_TI_FAST
#undef NTR_TI_MOTION
#undef NTR_TI_DEFORM

// The unit's launch under the shared path (trace_instanced_launch.h): stats != NULL launches the instrumented kernel.
int trace_instanced_deform_call(const TwoLevelCall& c)
{
    return two_level_trace(c, [&c](DeviceState* ds, hipStream_t s, unsigned int blocks) {
        InstancedParams p{};
        two_level_fill(p, c, ds);
        p.poolNodes = c.poolNodes; p.poolNodesBytes = (uint32_t)c.poolNodesBytes;
        InstancedExtras x{};
        two_level_fill_visibility(x, c, ds);
        InstancedMotion mo{};
        mo.keys = c.motion->d_motionKeys; mo.rayTimes = c.motion->d_rayTimes; mo.time = c.motion->time;
        mo.keysBytes = (uint32_t)std::min<int64_t>(c.motion->motionKeysBytes, kPoolMaxBytes);
        InstancedDeform df{};
        df.nodes1 = c.deform->d_poolNodes1; df.verts0 = c.deform->d_poolVertRows0; df.verts1 = c.deform->d_poolVertRows1;
        const dim3 grid(blocks), block(64);
        if (c.stats) hipLaunchKernelGGL(trace_instanced_deform_stats, grid, block, 0, s, p, x, mo, df);
        else hipLaunchKernelGGL(trace_instanced_deform, grid, block, 0, s, p, x, mo, df);
    });
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" int ntr_trace_instanced_deform(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results, int32_t* d_instanceIDs,
                                          const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink, const void* d_records,
                                          int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes, const void* d_poolTriWoop,
                                          int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex, const NtrInstanceVisibility* vis,
                                          const NtrInstanceMotion* motion, const NtrInstanceDeform* deform, float* seconds, void* stream)
{
    if (!deform)   // exactly the launch ntr_trace_instanced_motion makes
        return ntr_trace_instanced_motion(numRays, anyHit, d_rays, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records,
                                          numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, motion,
                                          seconds, stream);
    return trace_instanced_deform_call({"ntr_trace_instanced_deform", kTwoLevelBinary, TwoLevelSeed::kNone, nullptr, numRays, anyHit, d_rays, nullptr,
                                        -1, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records, numInstances, d_poolNodes,
                                        poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, nullptr, seconds, stream, nullptr,
                                        nullptr, motion, nullptr, deform, nullptr});
}

extern "C" int ntr_trace_instanced_deform_stats(int32_t numRays, int32_t anyHit, const NtrRay* d_rays, NtrRayResult* d_results,
                                                int32_t* d_instanceIDs, const void* d_tlasNodes, int64_t tlasNodesBytes, int32_t rootLink,
                                                const void* d_records, int32_t numInstances, const void* d_poolNodes, int64_t poolNodesBytes,
                                                const void* d_poolTriWoop, int64_t poolTriWoopBytes, const int32_t* d_poolTriIndex,
                                                const NtrInstanceVisibility* vis, const NtrInstanceMotion* motion,
                                                const NtrInstanceDeform* deform, NtrInstancedTraceStats* stats,
                                                NtrInstancedMotionStats* motionStats, NtrInstancedDeformStats* deformStats, void* stream)
{
    if (deformStats) memset(deformStats, 0, sizeof(*deformStats));
    if (!stats || !motionStats || !deformStats) {
        if (stats) memset(stats, 0, sizeof(*stats));
        if (motionStats) memset(motionStats, 0, sizeof(*motionStats));
        return set_error(NTR_ERR_INVALID, "ntr_trace_instanced_deform_stats: null stats");
    }
    if (!deform)   // the motion kernel's instrumented variant: nothing deforms, the three deform counters stay zero
        return ntr_trace_instanced_motion_stats(numRays, anyHit, d_rays, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records,
                                                numInstances, d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis,
                                                motion, stats, motionStats, stream);
    return trace_instanced_deform_call({"ntr_trace_instanced_deform_stats", kTwoLevelBinary, TwoLevelSeed::kNone, nullptr, numRays, anyHit, d_rays,
                                        nullptr, -1, d_results, d_instanceIDs, d_tlasNodes, tlasNodesBytes, rootLink, d_records, numInstances,
                                        d_poolNodes, poolNodesBytes, d_poolTriWoop, poolTriWoopBytes, d_poolTriIndex, vis, nullptr, nullptr, stream,
                                        stats, nullptr, motion, motionStats, deform, deformStats});
}
