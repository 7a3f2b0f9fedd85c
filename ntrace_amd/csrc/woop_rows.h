// woop_rows.h -- the Woop rows of one triangle (calcWoopKernel, emitTreeKernel.cu:574-635), shared by the LBVH and HLBVH builders.
#pragma once
#include <hip/hip_runtime.h>

namespace ntr {

// ---- Woop rows (emitTreeKernel.cu:574-635) ---------------------------------------------------------
__device__ __forceinline__ void woop_rows_verts(float v0x, float v0y, float v0z, float v1x, float v1y, float v1z, float v2x, float v2y,
                                                float v2z, float4& r0, float4& r1, float4& r2)
{
    const float c0x = v0x - v2x, c0y = v0y - v2y, c0z = v0z - v2z;
    const float c1x = v1x - v2x, c1y = v1y - v2y, c1z = v1z - v2z;
    const float c2x = c0y * c1z - c0z * c1y, c2y = c0z * c1x - c0x * c1z, c2z = c0x * c1y - c0y * c1x;
    const float den = c0x * (c2z * c1y - c1z * c2y) - c0y * (c2z * c1x - c1z * c2x) + c0z * (c2y * c1x - c1y * c2x);
    const float det = (float)(1.0 / (double)den);  // `1.0/(float)` is a binary64 divide in the reference (:589)

    const float i0x = (c2z * c1y - c1z * c2y) * det, i0y = -(c2z * c1x - c1z * c2x) * det, i0z = (c2y * c1x - c1y * c2x) * det;
    const float i1x = -(c2z * c0y - c0z * c2y) * det, i1y = (c2z * c0x - c0z * c2x) * det, i1z = -(c2y * c0x - c0y * c2x) * det;
    const float i2x = (c1z * c0y - c0z * c1y) * det, i2y = -(c1z * c0x - c0z * c1x) * det, i2z = (c1y * c0x - c0y * c1x) * det;
    const float o0w = -((-i2x) * v2x + (-i2y) * v2y + (-i2z) * v2z);
    const float o1w = (-i0x) * v2x + (-i0y) * v2y + (-i0z) * v2z;
    const float o2w = (-i1x) * v2x + (-i1y) * v2y + (-i1z) * v2z;
    float o0x = i2x;
    if (o0x == 0.0f) o0x = 0.0f;  // -0 would alias the leaf terminator
    r0 = make_float4(o0x, i2y, i2z, o0w);
    r1 = make_float4(i0x, i0y, i0z, o1w);
    r2 = make_float4(i1x, i1y, i1z, o2w);
}

__device__ __forceinline__ void woop_rows(const int* __restrict__ tri, const float* __restrict__ pos, int t, float4& r0, float4& r1,
                                          float4& r2)
{
    const int i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    woop_rows_verts(pos[3 * i0], pos[3 * i0 + 1], pos[3 * i0 + 2], pos[3 * i1], pos[3 * i1 + 1], pos[3 * i1 + 2], pos[3 * i2],
                    pos[3 * i2 + 1], pos[3 * i2 + 2], r0, r1, r2);
}

}  // namespace ntr
