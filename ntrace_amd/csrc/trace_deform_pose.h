// trace_deform_pose.h -- the pose of a deforming tree's words at a ray's time, stated once for the two units that trace such trees:
// trace_motion_kernels.hip over ONE Compact tree and trace_instanced_deform_kernels.hip over the deforming BLASes of a
// pool.  The rule is np_bvh_motion.deform_lerp.  trace_bvh_motion compiles to the code it had when its unit held these
// statements itself (scripts/kernel_isa_diff.sh).  Anonymous namespace, as trace_motion_pose.h: the kernels' names carry it.
#pragma once
#include <hip/hip_runtime.h>

namespace ntr {
namespace {

// deform_lerp of the spec, per word: the keys themselves at the two ends, both products rounded in between; u = 1.0f - t.
// NOT instance_motion.h's motion_lerp: no "same word" shortcut, so that the posed box contains the posed triangle exactly
__device__ __forceinline__ float motion_deform_lerp(float a, float b, float t, float u)
{
    const float v = u * a + t * b;
    return t == 0.0f ? a : (t == 1.0f ? b : v);
}
__device__ __forceinline__ float4 motion_deform_lerp4(const float4& a, const float4& b, float t, float u)
{
    return make_float4(motion_deform_lerp(a.x, b.x, t, u), motion_deform_lerp(a.y, b.y, t, u), motion_deform_lerp(a.z, b.z, t, u),
                       motion_deform_lerp(a.w, b.w, t, u));
}

}  // namespace
}  // namespace ntr
