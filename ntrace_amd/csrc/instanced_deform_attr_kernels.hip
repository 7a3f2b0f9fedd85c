// instanced_deform_attr_kernels.hip -- a two-level hit's attributes with the TRIANGLE at the ray's time too, for gfx950
// (ntr_instanced_hit_attributes_deform).
//
// An EXTENSION: the rule is the numpy spec tests/np_instanced_deform_frame.py (hit_attributes_deform), and the header comment of
// ntr_instanced_hit_attributes_deform (include/ntrace_amd.h) states the contract.  ntr_trace_instanced_deform poses a deforming BLAS's
// triangles at each ray's time; ntr_instanced_hit_attributes_motion forms the normal from key 0's vertices, which is the normal of a
// triangle the ray never met.  This is that call with one change: where the nine vertex words come from.
//   steps       instanced_attr.h's: the resolution with its range checks, the cross product over nine words, the transpose, the
//               normalisation; instanced_motion_attr_kernels.hip's moving test and instance_motion.h's pose, unchanged
//   deforming   the ray is resolved and d_blasDeforming[b] != 0, b = the instance's blas word, which the resolution has range checked
//   key 0       nine scalar loads from d_vtxPos for every shaded lane (12-byte rows: no wider load is aligned)
//   key 1       nine more from d_vtxPos1 at the same indices, and trace_deform_pose.h's motion_deform_lerp per word at the clamped
//               time: the vertex rows ntr_bvh_motion_refit writes are the vertices' words verbatim, so these are the words the trace
//               tested.  Nothing of d_vtxPos1 is read for a lane that is not deforming
//   votes       key 1 and the nine lerps sit behind __ballot(deforming) != 0, the instance's pose behind __ballot(moving) != 0 as
//               before: a wave whose hits are all on static instances of static BLASes runs ntr_instanced_hit_attributes' arithmetic
//               after two scalar branches
// One thread per ray, one 16-byte store per output.  No scratch, no read-back, no atomics: the call is capturable as it stands.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ntr_internal.h"
#include "instance_motion.h"
#include "instanced_attr.h"
#include "trace_deform_pose.h"

namespace ntr {
namespace {

static_assert(kMotionKeyBytes == 128 && kMotionKey1Bytes == 64, "a key entry is read as float4 0..2 (key 0) and 4..6 (key 1) of eight");

__device__ __forceinline__ bool same_words(float4 a, float4 b)
{
    return __float_as_uint(a.x) == __float_as_uint(b.x) && __float_as_uint(a.y) == __float_as_uint(b.y) &&
           __float_as_uint(a.z) == __float_as_uint(b.z) && __float_as_uint(a.w) == __float_as_uint(b.w);
}

__global__ __launch_bounds__(IHA_BLOCK) void instanced_hit_attributes_deform_kernel(
    int numRays, const int4* results, const int* __restrict__ instanceIDs, const NtrInstance* __restrict__ inst, int numInstances,
    const int2* __restrict__ blasTris, int numBlas, const int* __restrict__ triVtx, int numTrisTotal, const float* __restrict__ pos,
    const float* __restrict__ pos1, const uint32_t* __restrict__ blasDeforming, int numVerts, const float4* __restrict__ keys,
    const float* __restrict__ rayTimes, float time, int4* outResults, float4* __restrict__ normals)
{
    const unsigned int r = blockIdx.x * (unsigned int)IHA_BLOCK + threadIdx.x;   // < 2^31 + IHA_BLOCK
    if (r >= (unsigned int)numRays) return;
    const int4 res = results[r];             // (outResults may be results: this thread alone reads and writes record r)
    const int i = instanceIDs[r];
    int va, vb, vc;
    const int g = attr_resolve(res.x, i, inst, numInstances, blasTris, numBlas, triVtx, numTrisTotal, numVerts, va, vb, vc);
    const bool shade = g >= 0 && normals;    // (i is in [0, numInstances) then, and its blas word in [0, numBlas))
    float p[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float4 w0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), w1 = w0, w2 = w0;   // (a zero W gives the zero normal)
    float4 k0[3], k1[3];
    bool moving = false, deforming = false;
    if (shade) {
        attr_load_triangle(pos, va, vb, vc, p);
        deforming = blasDeforming[inst[i].blas] != 0u;
        const float4* e = keys + (kMotionKeyBytes / 16) * (size_t)i;
        k0[0] = e[0]; k0[1] = e[1]; k0[2] = e[2];
        k1[0] = e[kMotionKey1Bytes / 16]; k1[1] = e[kMotionKey1Bytes / 16 + 1]; k1[2] = e[kMotionKey1Bytes / 16 + 2];
        moving = !(same_words(k0[0], k1[0]) && same_words(k0[1], k1[1]) && same_words(k0[2], k1[2]));
        if (!moving) {
            const float4* w = reinterpret_cast<const float4*>(inst[i].worldToObject);
            w0 = w[0]; w1 = w[1]; w2 = w[2];
        }
    }
    // the wave votes twice: one whose hits are all on static instances of static BLASes goes on after two scalar branches
    if (__ballot(deforming) != 0ull && deforming) {
        const float t = motion_clamp_time(rayTimes ? rayTimes[r] : time);
        const float u = 1.0f - t;
        float q[9];
        attr_load_triangle(pos1, va, vb, vc, q);
#pragma unroll
        for (int k = 0; k < 9; k++) p[k] = motion_deform_lerp(p[k], q[k], t, u);
    }
    if (__ballot(moving) != 0ull && moving) {
        const float t = motion_clamp_time(rayTimes ? rayTimes[r] : time);
        motion_pose_keys(k0, k1, t, w0, w1, w2);   // (no inverse: the rows stay zero)
    }
    float ox, oy, oz;
    attr_cross(p, ox, oy, oz);
    if (outResults) outResults[r] = make_int4(g, res.y, res.z, res.w);
    if (normals) normals[r] = shade ? attr_world_normal(w0, w1, w2, ox, oy, oz) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_instanced_hit_attributes_deform(int32_t numRays, const NtrRayResult* d_results, const int32_t* d_instanceIDs,
                                        const NtrInstancedGeometry* geom, const NtrInstanceMotion* motion,
                                        const NtrInstancedDeformGeometry* deform, NtrRayResult* d_outResults, float* d_normals, void* stream)
{
    if (!deform)   // exactly the launch ntr_instanced_hit_attributes_motion makes
        return ntr_instanced_hit_attributes_motion(numRays, d_results, d_instanceIDs, geom, motion, d_outResults, d_normals, stream);
    const char* fn = "ntr_instanced_hit_attributes_deform";
    if (numRays < 0) return set_error(NTR_ERR_INVALID, "%s: numRays < 0", fn);
    if (numRays == 0) return NTR_OK;
    if (attr_check(fn, d_results, d_instanceIDs, geom, d_outResults, d_normals) != NTR_OK) return NTR_ERR_INVALID;
    if (motion && motion_check(fn, motion, geom->numInstances) != NTR_OK) return NTR_ERR_INVALID;
    if (!motion) return set_error(NTR_ERR_INVALID, "%s: null motion", fn);   // (the trace's rule and words)
    if (!deform->d_vtxPos1) return set_error(NTR_ERR_INVALID, "%s: null d_vtxPos1", fn);
    if (!deform->d_blasDeforming) return set_error(NTR_ERR_INVALID, "%s: null d_blasDeforming", fn);
    if (((uintptr_t)deform->d_vtxPos1 | (uintptr_t)deform->d_blasDeforming) & 3u)
        return set_error(NTR_ERR_INVALID, "%s: d_vtxPos1 and d_blasDeforming must be 4-byte aligned", fn);

    int dev = 0;
    NTR_HIP(hipGetDevice(&dev));
    hipLaunchKernelGGL(instanced_hit_attributes_deform_kernel, dim3((unsigned int)(((long long)numRays + IHA_BLOCK - 1) / IHA_BLOCK)),
                       dim3(IHA_BLOCK), 0, (hipStream_t)stream, (int)numRays, reinterpret_cast<const int4*>(d_results), d_instanceIDs,
                       geom->d_instances, (int)geom->numInstances, reinterpret_cast<const int2*>(geom->d_blasTris), (int)geom->numBlas,
                       geom->d_triVtxIndex, (int)geom->numTrisTotal, geom->d_vtxPos, deform->d_vtxPos1, deform->d_blasDeforming,
                       (int)geom->numVerts, reinterpret_cast<const float4*>(motion->d_motionKeys), motion->d_rayTimes, motion->time,
                       reinterpret_cast<int4*>(d_outResults), reinterpret_cast<float4*>(d_normals));
    NTR_HIP(hipGetLastError());
    return NTR_OK;
}

}  // extern "C"
