// tlas_world_box.h -- the world box of an instance from its BLAS's object box, stated once for the two top-level refits
// (tlas_refit_kernels.hip over the binary node 0, tlas_wide_refit_kernels.hip over the wide root's union).  The rule is
// np_instanced.instance_box: eight corners through objectToWorld, min / max in the total order, no padding.
#pragma once
#include <hip/hip_runtime.h>

#include "device_prims.h"

namespace ntr {

// xform's component (np_instanced.py): r = 0; r += a0 * x; r += a1 * y; r += a2 * z; r += a3 * w
__device__ __forceinline__ float tlr_dot4(const float* a, float x, float y, float z, float w)
{
    float r = 0.0f;
    r += a[0] * x;
    r += a[1] * y;
    r += a[2] * z;
    r += a[3] * w;
    return r;
}

// np_instanced.instance_box: n0, n1, nz are the first three float4 of the BLAS's node 0, m is objectToWorld
__device__ __forceinline__ void tlr_world_box(const float4& n0, const float4& n1, const float4& nz, const float (&m)[12], float (&wlo)[3],
                                              float (&whi)[3])
{
    // the object box: the union of node 0's child boxes (an empty child, (FLT_MAX, -FLT_MAX), drops out by itself)
    const float lo[3] = {ord_min(n0.x, n1.x), ord_min(n0.z, n1.z), ord_min(nz.x, nz.z)};
    const float hi[3] = {ord_max(n0.y, n1.y), ord_max(n0.w, n1.w), ord_max(nz.y, nz.w)};
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const float x = (c & 1) ? hi[0] : lo[0], y = (c & 2) ? hi[1] : lo[1], z = (c & 4) ? hi[2] : lo[2];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const float p = tlr_dot4(m + 4 * r, x, y, z, 1.0f);
            wlo[r] = c == 0 ? p : ord_min(wlo[r], p);
            whi[r] = c == 0 ? p : ord_max(whi[r], p);
        }
    }
}

}  // namespace ntr
