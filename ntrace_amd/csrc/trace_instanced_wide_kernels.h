// trace_instanced_wide_kernels.h -- what the two translation units of the two-level trace over 4-wide trees share: the kernels'
// parameters and the fetch.  trace_instanced_wide_kernels.hip holds the three unseeded kernels and the entry points,
// trace_instanced_wide_seeded_kernels.hip the seeded kernels.  Two units for the reason trace_instanced_kernels.h gives:
// the unseeded kernels must stay the kernels they were, instruction for instruction (scripts/kernel_isa_diff.sh).  The types stay in an
// anonymous namespace, which the unseeded kernels' names carry; the launcher of the other unit therefore takes them as bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntr_internal.h"
#include "instanced_wide_bvh.h"
#include "trace_lane.h"
#include "trace_wide_lane.h"

namespace ntr {

// trace_instanced_wide_seeded_kernels.hip: launches trace_instanced_wide_seeded<stats> over `blocks` workgroups of 64.  params, seed: an
// InstancedWideParams and an InstancedWideSeed of the caller's unit.
void launch_trace_instanced_wide_seeded(bool stats, unsigned int blocks, hipStream_t stream, const void* params, const void* seed);

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
// What the seeded kernels take beside InstancedWideParams, which stays as the unseeded kernels have it: one result record per ray to
// start from (tests/np_instanced_seeded.py).
struct InstancedWideSeed {
    const NtrRayResult* seedResults;   // numRays records, 16-byte aligned; may be InstancedWideParams::results
    int32_t seedInstance;              // the instance id of a ray that keeps a seed that is a hit
};

}  // namespace
}  // namespace ntr
