// instanced_motion_attr_kernels.hip -- a two-level hit's attributes with the normal at the RAY'S time, for gfx950
// (ntr_instanced_hit_attributes_motion).
//
// An EXTENSION: the rule is the numpy spec tests/np_instanced_motion_frame.py (hit_attributes_motion), and the header comment of
// ntr_instanced_hit_attributes_motion (include/ntrace_amd.h) states the contract.  ntr_trace_instanced_motion poses a moving instance
// at each ray's time; ntr_instanced_hit_attributes forms the normal from key 0's worldToObject, which is wrong for an instance that
// turns inside the shutter.  This is that call with one change: where W comes from.
//   steps       instanced_attr.h's: the resolution with its range checks, the object-space cross product, the transpose, the
//               normalisation
//   moving      words 0..11 and 16..27 of the instance's 128-byte key entry differ bitwise (six 16-byte loads; the host has checked
//               that the key buffer holds an entry for every instance, and only a resolved ray's instance is read).  This call has
//               no records, so it cannot read the trace's word 15; the two say the same of a buffer ntr_tlas_motion_refit wrote
//   pose        instance_motion.h's, the trace's own: twelve lerps at the clamped time and the binary64 inverse.  No inverse: the id
//               stays resolved and the normal is (0, 0, 0, 0)
//   vote        the pose sits behind __ballot(moving) != 0: a wave whose hits are all on static instances runs
//               ntr_instanced_hit_attributes' arithmetic after one scalar branch; the binary64 registers are live inside it only
// One thread per ray, one 16-byte store per output.  No scratch, no read-back, no atomics: the call is capturable as it stands.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ntr_internal.h"
#include "instance_motion.h"
#include "instanced_attr.h"

namespace ntr {
namespace {

static_assert(kMotionKeyBytes == 128 && kMotionKey1Bytes == 64, "a key entry is read as float4 0..2 (key 0) and 4..6 (key 1) of eight");

__device__ __forceinline__ bool same_words(float4 a, float4 b)
{
    return __float_as_uint(a.x) == __float_as_uint(b.x) && __float_as_uint(a.y) == __float_as_uint(b.y) &&
           __float_as_uint(a.z) == __float_as_uint(b.z) && __float_as_uint(a.w) == __float_as_uint(b.w);
}

__global__ __launch_bounds__(IHA_BLOCK) void instanced_hit_attributes_motion_kernel(
    int numRays, const int4* results, const int* __restrict__ instanceIDs, const NtrInstance* __restrict__ inst, int numInstances,
    const int2* __restrict__ blasTris, int numBlas, const int* __restrict__ triVtx, int numTrisTotal, const float* __restrict__ pos, int numVerts,
    const float4* __restrict__ keys, const float* __restrict__ rayTimes, float time, int4* outResults, float4* __restrict__ normals)
{
    const unsigned int r = blockIdx.x * (unsigned int)IHA_BLOCK + threadIdx.x;   // < 2^31 + IHA_BLOCK
    if (r >= (unsigned int)numRays) return;
    const int4 res = results[r];             // (outResults may be results: this thread alone reads and writes record r)
    const int i = instanceIDs[r];
    int va, vb, vc;
    const int g = attr_resolve(res.x, i, inst, numInstances, blasTris, numBlas, triVtx, numTrisTotal, numVerts, va, vb, vc);
    const bool shade = g >= 0 && normals;    // (i is in [0, numInstances) then: its row and its key entry are there)
    float ox = 0.0f, oy = 0.0f, oz = 0.0f;
    float4 w0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), w1 = w0, w2 = w0;   // (a zero W gives the zero normal)
    float4 k0[3], k1[3];
    bool moving = false;
    if (shade) {
        attr_object_normal(pos, va, vb, vc, ox, oy, oz);
        const float4* e = keys + (kMotionKeyBytes / 16) * (size_t)i;
        k0[0] = e[0]; k0[1] = e[1]; k0[2] = e[2];
        k1[0] = e[kMotionKey1Bytes / 16]; k1[1] = e[kMotionKey1Bytes / 16 + 1]; k1[2] = e[kMotionKey1Bytes / 16 + 2];
        moving = !(same_words(k0[0], k1[0]) && same_words(k0[1], k1[1]) && same_words(k0[2], k1[2]));
        if (!moving) {
            const float4* w = reinterpret_cast<const float4*>(inst[i].worldToObject);
            w0 = w[0]; w1 = w[1]; w2 = w[2];
        }
    }
    // the wave votes: one whose hits are all on static instances goes on after one scalar branch
    if (__ballot(moving) != 0ull && moving) {
        const float t = motion_clamp_time(rayTimes ? rayTimes[r] : time);
        motion_pose_keys(k0, k1, t, w0, w1, w2);   // (no inverse: the rows stay zero)
    }
    if (outResults) outResults[r] = make_int4(g, res.y, res.z, res.w);
    if (normals) normals[r] = shade ? attr_world_normal(w0, w1, w2, ox, oy, oz) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

}  // namespace
}  // namespace ntr

using namespace ntr;

extern "C" {

int ntr_instanced_hit_attributes_motion(int32_t numRays, const NtrRayResult* d_results, const int32_t* d_instanceIDs,
                                        const NtrInstancedGeometry* geom, const NtrInstanceMotion* motion, NtrRayResult* d_outResults,
                                        float* d_normals, void* stream)
{
    if (!motion)   // exactly the launch ntr_instanced_hit_attributes makes
        return ntr_instanced_hit_attributes(numRays, d_results, d_instanceIDs, geom, d_outResults, d_normals, stream);
    const char* fn = "ntr_instanced_hit_attributes_motion";
    if (numRays < 0) return set_error(NTR_ERR_INVALID, "%s: numRays < 0", fn);
    if (numRays == 0) return NTR_OK;
    if (attr_check(fn, d_results, d_instanceIDs, geom, d_outResults, d_normals) != NTR_OK) return NTR_ERR_INVALID;
    if (motion_check(fn, motion, geom->numInstances) != NTR_OK) return NTR_ERR_INVALID;

    int dev = 0;
    NTR_HIP(hipGetDevice(&dev));
    hipLaunchKernelGGL(instanced_hit_attributes_motion_kernel, dim3((unsigned int)(((long long)numRays + IHA_BLOCK - 1) / IHA_BLOCK)),
                       dim3(IHA_BLOCK), 0, (hipStream_t)stream, (int)numRays, reinterpret_cast<const int4*>(d_results), d_instanceIDs,
                       geom->d_instances, (int)geom->numInstances, reinterpret_cast<const int2*>(geom->d_blasTris), (int)geom->numBlas,
                       geom->d_triVtxIndex, (int)geom->numTrisTotal, geom->d_vtxPos, (int)geom->numVerts,
                       reinterpret_cast<const float4*>(motion->d_motionKeys), motion->d_rayTimes, motion->time,
                       reinterpret_cast<int4*>(d_outResults), reinterpret_cast<float4*>(d_normals));
    NTR_HIP(hipGetLastError());
    return NTR_OK;
}

}  // extern "C"
