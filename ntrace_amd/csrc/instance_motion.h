// instance_motion.h -- the pose of a moving instance at a ray's time, stated once for the units that need it
// (trace_instanced_motion_kernels.hip, instanced_motion_attr_kernels.hip; the rule is tests/np_instanced_motion.py:
// clamp_time, lerp, invert_many).  The arithmetic only: each unit loads the two keys its own way (the trace through a range-checked
// descriptor, the attributes through checked 16-byte loads) and hands them over in registers.  Binary32 lerps with both products
// rounded -- whatever includes this is compiled without contraction -- and instance_math.h's binary64 inverse.
#pragma once
#include <hip/hip_runtime.h>

#include "ntr_internal.h"
#include "instance_math.h"
#include "instanced_bvh.h"

namespace ntr {

// the ray's time as every motion kernel uses it: t > 0 ? (t < 1 ? t : 1) : 0, so a NaN gives 0
__device__ __forceinline__ float motion_clamp_time(float t) { return t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f; }

// M(t) component (tests/np_instanced_motion.py, lerp): the keys themselves at the two ends and wherever they are the same word
__device__ __forceinline__ float motion_lerp(float a, float b, float t, float u)
{
    const float v = u * a + t * b;   // (both products rounded: the library is built without contraction)
    return (t == 0.0f || __float_as_uint(a) == __float_as_uint(b)) ? a : (t == 1.0f ? b : v);
}

// worldToObject(t) of the keys k0, k1 (three rows of objectToWorld each) into the rows a, b, c; false, and the rows untouched, where
// M(t) has no inverse
__device__ __forceinline__ bool motion_pose_keys(const float4 (&k0)[3], const float4 (&k1)[3], float t, float4& a, float4& b, float4& c)
{
    const float u = 1.0f - t;
    float m[12], w[12];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        m[4 * r + 0] = motion_lerp(k0[r].x, k1[r].x, t, u);
        m[4 * r + 1] = motion_lerp(k0[r].y, k1[r].y, t, u);
        m[4 * r + 2] = motion_lerp(k0[r].z, k1[r].z, t, u);
        m[4 * r + 3] = motion_lerp(k0[r].w, k1[r].w, t, u);
    }
    if (!instance_invert(m, w)) return false;
    a = make_float4(w[0], w[1], w[2], w[3]);
    b = make_float4(w[4], w[5], w[6], w[7]);
    c = make_float4(w[8], w[9], w[10], w[11]);
    return true;
}

// What every call that takes an NtrInstanceMotion refuses, before any device work: NTR_OK, or the error set under the caller's name
inline int motion_check(const char* fn, const NtrInstanceMotion* motion, int64_t numInstances)
{
    if ((((uintptr_t)motion->d_rayTimes) & 3u) != 0) return set_error(NTR_ERR_INVALID, "%s: the ray times must be 4-byte aligned", fn);
    if (!motion->d_motionKeys || (((uintptr_t)motion->d_motionKeys) & 15u) != 0)
        return set_error(NTR_ERR_INVALID, "%s: the motion keys (ntr_tlas_motion_refit) must be given and 16-byte aligned", fn);
    if (motion->motionKeysBytes < (int64_t)kMotionKeyBytes * numInstances)
        return set_error(NTR_ERR_INVALID, "%s: motionKeysBytes below 128 * numInstances", fn);
    return NTR_OK;
}

}  // namespace ntr
