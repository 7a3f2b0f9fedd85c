// trace_motion_pose.h -- what the two motion trace units share beside the arithmetic of instance_motion.h: the kernels' motion
// parameters and the load of a moving instance's two keys (trace_instanced_motion_kernels.hip over the binary trees, DESIGN.md 6aa;
// trace_instanced_wide_motion_kernels.hip over the 4-wide trees).  The motion key buffer does not depend on the tree's
// width, so the pose is stated once; the binary unit's two kernels compile to the code they had when the unit held these statements
// itself (scripts/kernel_isa_diff.sh).  The types stay in an anonymous namespace, which the kernels' names carry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntr_internal.h"
#include "instance_motion.h"
#include "instanced_bvh.h"
#include "trace_lane.h"

namespace ntr {
namespace {

// What the motion kernels take beside their unit's parameters
struct InstancedMotion {
    const void* keys;          // the motion key buffer: 128 bytes per instance (instanced_bvh.h)
    const float* rayTimes;     // numRays words, or NULL: every ray has `time`
    uint32_t keysBytes;        // the descriptor's range
    float time;
};

// worldToObject(t) of moving instance idx into the rows a, b, c; false, and the rows untouched, where M(t) has no inverse.  The loads
// are here; the lerps and the inverse are instance_motion.h's, shared with instanced_motion_attr_kernels.hip
__device__ __forceinline__ bool motion_pose(Rsrc rKeys, int idx, float t, float4& a, float4& b, float4& c)
{
    // 128 * idx may pass 2^32 for an index no key buffer can hold (a descriptor ends below 2^32): such a lane reads nothing
    const int ofs = (unsigned)idx < (unsigned)(kPoolMaxBytes / kMotionKeyBytes) ? idx * kMotionKeyBytes : kNoNode;
    const float4 k0[3] = {ld4(rKeys, ofs), ld4(rKeys, ofs + 16), ld4(rKeys, ofs + 32)};
    const float4 k1[3] = {ld4(rKeys, ofs + kMotionKey1Bytes), ld4(rKeys, ofs + kMotionKey1Bytes + 16), ld4(rKeys, ofs + kMotionKey1Bytes + 32)};
    return motion_pose_keys(k0, k1, t, a, b, c);
}

}  // namespace
}  // namespace ntr
