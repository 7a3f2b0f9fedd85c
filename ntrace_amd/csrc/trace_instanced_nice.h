// trace_instanced_nice.h -- what the FAST two-level kernels share (trace_instanced_fast_kernels.hip over binary trees, DESIGN.md 6w;
// trace_instanced_wide_fast_kernels.hip over 4-wide trees): the flag words they are handed and the per-lane `nice`,
// stated once.  The helpers stay in an anonymous namespace, as they were in trace_instanced_fast_kernels.hip: that unit's kernels are
// the kernels they were, instruction for instruction (scripts/kernel_isa_diff.sh).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntr_internal.h"
#include "trace_lane.h"

namespace ntr {
namespace {

struct InstancedFast {
    const uint32_t* flags;   // ntr_instanced_validate's (ntr_instanced_wide_validate's) four words: [0] withheld on the top level, [1] in the pool
};

// `nice` of ray r on a level whose withheld bits are `held`; a nice ray gets its reciprocals (load_ray's, trace_lane.h)
__device__ __forceinline__ bool level_nice(RayRegs& r, unsigned int held)
{
    const bool nice = !(held & NTR_BVH_FASTDIV) && ray_is_nice(r, ~held);
    if (nice) { r.rx = exact_rcp(r.dx); r.ry = exact_rcp(r.dy); r.rz = exact_rcp(r.dz); }
    return nice;
}

// How a kernel whose instrumentation is a template parameter holds `nice`: a bool, or -- PIN, the instrumented variants -- a word pinned
// to a vector register, as trace_instanced_body.h's NTR_TI_NICE_PIN has it: as a lane mask in a scalar pair it is an SGPR spill there
template <bool PIN>
struct NiceWord {
    typedef bool type;
    static __device__ __forceinline__ void pin(bool&) {}
};
template <>
struct NiceWord<true> {
    typedef unsigned int type;
    static __device__ __forceinline__ void pin(unsigned int& v) { keep(v); }
};

}  // namespace
}  // namespace ntr
