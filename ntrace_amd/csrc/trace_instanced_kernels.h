// trace_instanced_kernels.h -- what the translation units of the two-level trace share: the kernels' parameters and the fetch.
// trace_instanced_kernels.hip holds the unmasked kernel and the entry points, trace_instanced_masked_kernels.hip the masked and the
// instrumented kernel, trace_instanced_seeded_kernels.hip the two seeded kernels.  Separate units because the unmasked kernel must stay the kernel it was, instruction for instruction
// (scripts/kernel_isa_diff.sh): with further kernels in its unit hipcc compiles it differently (an integer compare where it had a class
// test, another register allocation), and that would have to be measured again.  The types stay in an anonymous namespace, which the
// unmasked kernel's name carries; the launcher of the other unit therefore takes them as bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntr_internal.h"
#include "instanced_bvh.h"
#include "trace_lane.h"

namespace ntr {

// trace_instanced_masked_kernels.hip: launches trace_instanced_stats (stats) or trace_instanced_masked over `blocks` workgroups of 64.
// params, extras: an InstancedParams and an InstancedExtras of the caller's unit.
void launch_trace_instanced_variant(bool stats, unsigned int blocks, hipStream_t stream, const void* params, const void* extras);
// trace_instanced_seeded_kernels.hip: launches trace_instanced_seeded_stats (stats) or trace_instanced_seeded; seed: an InstancedSeed.
void launch_trace_instanced_seeded(bool stats, unsigned int blocks, hipStream_t stream, const void* params, const void* extras, const void* seed);

namespace {

struct InstancedParams {
    int32_t numRays, anyHit;
    const NtrRay* rays;
    NtrRayResult* results;
    int32_t* instanceIDs;
    const void *tlas, *records, *poolNodes, *poolWoop;
    uint32_t tlasBytes, recordsBytes, poolNodesBytes, poolWoopBytes;   // descriptor ranges (out-of-range loads return 0)
    const int32_t* triIndex;
    int32_t rootLink, numInstances;
    unsigned int* status;   // sticky error bits
};
// What the masked and the instrumented kernel take beside InstancedParams, which stays as the unmasked kernel has it.
struct InstancedExtras {
    const void* instMasks;         // numInstances words, or NULL: every instance 0xFFFFFFFF
    const uint32_t* rayMasks;      // numRays words, or NULL: every ray has rayMask
    uint32_t instMasksBytes, rayMask;
    unsigned long long* stats;     // STATS: {top inner, entries, masked, inner, triangle tests, leaf terminators, hits}; the fast variants
                                   // (NTR_TI_FAST) add [8..11] = {wave steps, FAST wave steps, nice starts, nice entries}
};
struct InstancedLaneStats {
    unsigned int topInner, entries, masked, inner, tris, leaves;
};
// What the seeded kernels take beside the two: one result record per ray to start from (tests/np_instanced_seeded.py).
struct InstancedSeed {
    const NtrRayResult* seedResults;   // numRays records, 16-byte aligned; may be InstancedParams::results
    int32_t seedInstance;              // the instance id of a ray that keeps a seed that is a hit
};

// Lanes of mask k fetch 64 B at byte offset `ofs` of buffer k (range-checked: beyond the extent a load returns 0 and touches no memory),
// all into the same registers; a buffer whose mask is empty is skipped by a scalar branch; the other lanes keep what a..d held.
#define NTR_FETCH64_GROUP(R, M, L)                                          \
    "s_and_b64 exec, %[sav], %[" M "]\n\t"                                  \
    "s_cbranch_execz .Lcs_fetch" L "%=\n\t"                                 \
    "buffer_load_dwordx4 %[a], %[ofs], %[" R "], 0 offen\n\t"               \
    "buffer_load_dwordx4 %[b], %[ofs], %[" R "], 0 offen offset:16\n\t"     \
    "buffer_load_dwordx4 %[c], %[ofs], %[" R "], 0 offen offset:32\n\t"     \
    "buffer_load_dwordx4 %[d], %[ofs], %[" R "], 0 offen offset:48\n\t"     \
    ".Lcs_fetch" L "%=:\n\t"
__device__ __forceinline__ void fetch64_four_buffers(u32x4 r0, u32x4 r1, u32x4 r2, u32x4 r3, int ofs, unsigned long long m0,
                                                     unsigned long long m1, unsigned long long m2, unsigned long long m3, float4& a, float4& b,
                                                     float4& c, float4& d)
{
    u32x4 va = as_u4(a), vb = as_u4(b), vc = as_u4(c), vd = as_u4(d);
    unsigned long long sav;
    asm volatile("s_mov_b64 %[sav], exec\n\t"
                 NTR_FETCH64_GROUP("r0", "m0", "a")
                 NTR_FETCH64_GROUP("r1", "m1", "b")
                 NTR_FETCH64_GROUP("r2", "m2", "c")
                 NTR_FETCH64_GROUP("r3", "m3", "d")
                 "s_mov_b64 exec, %[sav]\n\t"
                 "s_waitcnt vmcnt(0)"
                 : [a] "+v"(va), [b] "+v"(vb), [c] "+v"(vc), [d] "+v"(vd), [sav] "=&s"(sav)
                 : [ofs] "v"(ofs), [r0] "s"(r0), [r1] "s"(r1), [r2] "s"(r2), [r3] "s"(r3), [m0] "s"(m0), [m1] "s"(m1), [m2] "s"(m2), [m3] "s"(m3)
                 : "memory", "scc");   // (s_and_b64 writes SCC)
    a = as_f4(va); b = as_f4(vb); c = as_f4(vc); d = as_f4(vd);
}
// ... and the lanes of mask m4 (the entering lanes, or none) fetch the word at byte offset `wofs` of a fifth buffer into w: issued with
// the other groups, under the same saved exec, and waited for in the same s_waitcnt -- no second round trip for an entering step.
__device__ __forceinline__ void fetch64_four_buffers_and_word(u32x4 r0, u32x4 r1, u32x4 r2, u32x4 r3, u32x4 r4, int ofs, int wofs,
                                                              unsigned long long m0, unsigned long long m1, unsigned long long m2,
                                                              unsigned long long m3, unsigned long long m4, float4& a, float4& b, float4& c,
                                                              float4& d, unsigned int& w)
{
    u32x4 va = as_u4(a), vb = as_u4(b), vc = as_u4(c), vd = as_u4(d);
    unsigned long long sav;
    asm volatile("s_mov_b64 %[sav], exec\n\t"
                 NTR_FETCH64_GROUP("r0", "m0", "a")
                 NTR_FETCH64_GROUP("r1", "m1", "b")
                 "s_and_b64 exec, %[sav], %[m4]\n\t"
                 "s_cbranch_execz .Lcs_fetchw%=\n\t"
                 "buffer_load_dword %[w], %[wofs], %[r4], 0 offen\n\t"
                 ".Lcs_fetchw%=:\n\t"
                 NTR_FETCH64_GROUP("r2", "m2", "c")
                 NTR_FETCH64_GROUP("r3", "m3", "d")
                 "s_mov_b64 exec, %[sav]\n\t"
                 "s_waitcnt vmcnt(0)"
                 : [a] "+v"(va), [b] "+v"(vb), [c] "+v"(vc), [d] "+v"(vd), [w] "+v"(w), [sav] "=&s"(sav)
                 : [ofs] "v"(ofs), [wofs] "v"(wofs), [r0] "s"(r0), [r1] "s"(r1), [r2] "s"(r2), [r3] "s"(r3), [r4] "s"(r4), [m0] "s"(m0), [m1] "s"(m1),
                   [m2] "s"(m2), [m3] "s"(m3), [m4] "s"(m4)
                 : "memory", "scc");   // (s_and_b64 writes SCC)
    a = as_f4(va); b = as_f4(vb); c = as_f4(vc); d = as_f4(vd);
}
#undef NTR_FETCH64_GROUP
}  // namespace
}  // namespace ntr
