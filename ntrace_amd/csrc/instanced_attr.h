// instanced_attr.h -- the steps of a two-level hit's attributes, stated once for the units that resolve hits
// (instanced_attr_kernels.hip: ntr_instanced_hit_attributes; instanced_motion_attr_kernels.hip: ntr_instanced_hit_attributes_motion;
// instanced_deform_attr_kernels.hip: ntr_instanced_hit_attributes_deform; the rule is
// tests/np_instanced_frame.py).  The units differ in where worldToObject and the nine vertex words come from and in nothing else: the
// resolution with its range checks, the object-space normal, the transpose and the normalisation are here, and so are the refusals the
// entry points share, worded once with the caller's name.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ntr_internal.h"

namespace ntr {

constexpr int IHA_BLOCK = 256;
static_assert(sizeof(NtrInstance) == 112 && offsetof(NtrInstance, worldToObject) == 48 && offsetof(NtrInstance, blas) == 96,
              "the instance row is read as three 16-byte loads at byte 48 and a word at byte 96");
static_assert(sizeof(NtrBlasTris) == 8, "NtrBlasTris is read as one 8-byte load");

// The pool triangle g = firstTri + id of a hit and its three vertex indices, or -1 where the ray is not resolved.  Every index is
// range checked before it is used.
__device__ __forceinline__ int attr_resolve(int id, int i, const NtrInstance* __restrict__ inst, int numInstances, const int2* __restrict__ blasTris,
                                            int numBlas, const int* __restrict__ triVtx, int numTrisTotal, int numVerts, int& va, int& vb, int& vc)
{
    if (id >= 0 && i >= 0 && i < numInstances) {
        const int b = inst[i].blas;
        if (b >= 0 && b < numBlas) {
            const int2 bt = blasTris[b];     // (firstTri, numTris)
            const long long gg = (long long)bt.x + id;
            if (id < bt.y && gg >= 0 && gg < numTrisTotal) {
                va = triVtx[3 * (size_t)gg], vb = triVtx[3 * (size_t)gg + 1], vc = triVtx[3 * (size_t)gg + 2];
                if (va >= 0 && va < numVerts && vb >= 0 && vb < numVerts && vc >= 0 && vc < numVerts) return (int)gg;
            }
        }
    }
    return -1;
}

// a triangle's nine vertex words, a.xyz b.xyz c.xyz: 12-byte rows, so nine scalar loads
__device__ __forceinline__ void attr_load_triangle(const float* __restrict__ pos, int va, int vb, int vc, float (&p)[9])
{
    const float* pa = pos + 3 * (size_t)va;
    const float* pb = pos + 3 * (size_t)vb;
    const float* pc = pos + 3 * (size_t)vc;
    p[0] = pa[0], p[1] = pa[1], p[2] = pa[2];
    p[3] = pb[0], p[4] = pb[1], p[5] = pb[2];
    p[6] = pc[0], p[7] = pc[1], p[8] = pc[2];
}

// the object-space normal of nine vertex words (Scene.cpp:112's cross product)
__device__ __forceinline__ void attr_cross(const float (&p)[9], float& ox, float& oy, float& oz)
{
    const float ax = p[0], ay = p[1], az = p[2];
    const float e1x = p[3] - ax, e1y = p[4] - ay, e1z = p[5] - az;
    const float e2x = p[6] - ax, e2y = p[7] - ay, e2z = p[8] - az;
    ox = e1y * e2z - e1z * e2y, oy = e1z * e2x - e1x * e2z, oz = e1x * e2y - e1y * e2x;
}

// the object-space normal of a triangle of `pos`
__device__ __forceinline__ void attr_object_normal(const float* __restrict__ pos, int va, int vb, int vc, float& ox, float& oy, float& oz)
{
    float p[9];
    attr_load_triangle(pos, va, vb, vc, p);
    attr_cross(p, ox, oy, oz);
}

// through the transpose of worldToObject's linear part (rows w0, w1, w2): the inverse transpose of objectToWorld; (0, 0, 0, 0) where the
// length is zero or not finite
__device__ __forceinline__ float4 attr_world_normal(float4 w0, float4 w1, float4 w2, float ox, float oy, float oz)
{
    const float wx = (w0.x * ox + w1.x * oy) + w2.x * oz;
    const float wy = (w0.y * ox + w1.y * oy) + w2.y * oz;
    const float wz = (w0.z * ox + w1.z * oy) + w2.z * oz;
    const float l2 = (wx * wx + wy * wy) + wz * wz;
    if (l2 > 0.0f && l2 < __builtin_inff()) {   // (a NaN fails both)
        const float inv = 1.0f / sqrtf(l2);
        return make_float4(wx * inv, wy * inv, wz * inv, 1.0f);
    }
    return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// What both entry points refuse, before any device work (numRays > 0): NTR_OK, or the error set under the caller's name
inline int attr_check(const char* fn, const NtrRayResult* d_results, const int32_t* d_instanceIDs, const NtrInstancedGeometry* geom,
                      NtrRayResult* d_outResults, float* d_normals)
{
    if (!geom) return set_error(NTR_ERR_INVALID, "%s: geom is null", fn);
    if (!geom->d_instances || !geom->d_blasTris || !geom->d_triVtxIndex || !geom->d_vtxPos)
        return set_error(NTR_ERR_INVALID, "%s: a null pointer in geom (d_instances, d_blasTris, d_triVtxIndex and d_vtxPos are all needed)", fn);
    if (geom->numInstances < 1 || geom->numBlas < 1 || geom->numTrisTotal < 1 || geom->numVerts < 1)
        return set_error(NTR_ERR_INVALID, "%s: numInstances, numBlas, numTrisTotal and numVerts must all be >= 1", fn);
    if (!d_results || !d_instanceIDs) return set_error(NTR_ERR_INVALID, "%s: d_results or d_instanceIDs is null", fn);
    if (!d_outResults && !d_normals) return set_error(NTR_ERR_INVALID, "%s: both outputs are null (pass d_outResults, d_normals or both)", fn);
    if (((uintptr_t)d_results | (uintptr_t)d_outResults | (uintptr_t)d_normals | (uintptr_t)geom->d_instances) & 15u)
        return set_error(NTR_ERR_INVALID, "%s: d_results, d_outResults, d_normals and geom->d_instances must be 16-byte aligned", fn);
    if (((uintptr_t)geom->d_blasTris) & 7u) return set_error(NTR_ERR_INVALID, "%s: geom->d_blasTris must be 8-byte aligned", fn);
    return NTR_OK;
}

}  // namespace ntr
